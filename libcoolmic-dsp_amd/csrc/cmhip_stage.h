// cmhip_stage.h -- a stage object beside the batch, on the HIP side (not part of the C ABI; cmhip_engine.h includes it
// once fail and HIP_TRY exist): the ring a run's counts travel through, the device / stream / counts every stage owns
// (cmhip_src.hip, cmhip_mix.hip, cmhip_bus.hip, cmhip_lim.hip, cmhip_dyn.hip, cmhip_split.hip, cmhip_delay.hip, cmhip_agc.hip, cmhip_iir.hip embed StageBase), and the refusals of csrc/stage_io.h's
// checks as the caller reads them in cmhip_last_error().
#pragma once

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

// What a stage owns beside its own tables: its device, the stream its runs are ordered on (the caller's, or one of
// its own) and a run's counts on the device with the ring they arrive through.
struct CMHIP_INTERNAL StageBase {
    int         device = 0;
    hipStream_t stream = nullptr;
    bool        own_stream = false;
    uint32_t   *d_counts = nullptr;                  // [count_words] a run's counts, per stream
    CountsRing  counts;                              // ... on their way there

    int open(int dev, void *hip_stream, size_t count_words)
    {
        device = dev;
        HIP_TRY(hipSetDevice(device));
        if (hip_stream) {
            stream = (hipStream_t)hip_stream;
        } else {
            HIP_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
            own_stream = true;
        }
        HIP_TRY(hipMalloc((void **)&d_counts, count_words * sizeof(uint32_t)));
        HIP_TRY(counts.init(count_words));
        return COOLMIC_ERROR_NONE;
    }
    // (also of an object whose creation failed half way.)  The stream is synchronised before anything is freed, here
    // and by the caller: what the stage owns itself it frees after close(), with the device still current.
    void close()
    {
        (void)hipSetDevice(device);
        if (stream)
            (void)hipStreamSynchronize(stream);
        (void)hipFree(d_counts);
        counts.destroy();
        if (own_stream)
            (void)hipStreamDestroy(stream);
    }
};

// the body of cmhip_*_sync (m may be NULL)
static inline int stage_sync(StageBase *m, const char *who)
{
    if (!m)
        return fail(COOLMIC_ERROR_FAULT, "%s: NULL argument", who);
    HIP_TRY(hipSetDevice(m->device));
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

}  // namespace cmhip
