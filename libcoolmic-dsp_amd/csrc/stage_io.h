// stage_io.h -- what every object that runs over the slots of device arrays checks before it touches anything
// (include/coolmic_hip.h: the stage objects beside the batch, and the batch's "stream -1 means every stream"): the range
// of streams a call names, a run's pointers, strides and counts, and which of a history's two slots a run reads.  Host
// only, plain C++17, no HIP: tests/cpp/stage_io_test.cpp compiles it with g++ alone.  Nothing is dereferenced but the
// counts.
#ifndef CMHIP_STAGE_IO_H
#define CMHIP_STAGE_IO_H

#include <stddef.h>
#include <stdint.h>

namespace cmhip {

// `stream` of a call that takes one stream or, with -1, all of them: streams lo .. lo + n - 1
struct StreamRange {
    bool     ok;               // -1 or 0 .. streams - 1
    uint32_t lo, n;
};
static inline StreamRange stream_range(long stream, unsigned streams)
{
    if (stream == -1)
        return {true, 0u, streams};
    if (stream < 0 || (unsigned long)stream >= streams)
        return {false, 0u, 0u};
    return {true, (uint32_t)stream, 1u};
}

// the frames of stream s in a run: its count, or `frames` where the run has no counts
static inline uint32_t stage_count(const uint32_t *frames_per_stream, size_t s, size_t frames)
{
    return frames_per_stream ? frames_per_stream[s] : (uint32_t)frames;
}

// Which of the two slots of a per-stream history [2][streams][per] a run reads: slot `parity`.  The kernel writes the
// other slot and the host flips the parity after the launch, so the next run reads what this one wrote.
struct HistorySlots {
    size_t   streams = 0;
    unsigned parity = 0;
    // the element where stream s begins in the slot the next run reads
    size_t at(size_t s, size_t per) const { return ((size_t)parity * streams + s) * per; }
    void flip() { parity ^= 1u; }
};

// A run: in_slots slots of in_stride int16 samples at `in`, out_slots slots of out_stride samples at `out`.  Every
// input slot holds `frames` frames of in_channels samples, every output slot out_frames frames of out_channels.
enum StageOverlap : int {
    STAGE_APART = 0,           // the byte ranges of the two arrays may not share a byte
    STAGE_NOT_IN_PLACE,        // in == out is refused and nothing else (the resampler's documented rule)
};
struct StageRun {
    const void     *in, *out;
    size_t          in_stride, out_stride;
    size_t          frames, max_frames;
    const uint32_t *counts;    // [in_slots] frames per input slot, or nullptr: every slot has `frames`
    size_t          in_slots, out_slots;
    size_t          in_channels, out_frames, out_channels;
    StageOverlap    overlap;
};

enum StageRunError : int {
    STAGE_RUN_OK = 0,
    STAGE_RUN_NULL,            // in or out is NULL
    STAGE_RUN_ALIGN,           // in or out is not 16-byte aligned
    STAGE_RUN_STRIDE8,         // a stride is no multiple of 8 samples
    STAGE_RUN_FRAMES,          // frames above max_frames
    STAGE_RUN_COUNT,           // a count above frames                              (*where: the slot)
    STAGE_RUN_IN_STRIDE,       // in_stride below frames * in_channels
    STAGE_RUN_OUT_STRIDE,      // out_stride below out_frames * out_channels
    STAGE_RUN_SPAN,            // an array of slots * stride samples would end past the address space
    STAGE_RUN_OVERLAP,         // the overlap rule
};

// the end of [base, base + slots * stride * sizeof(int16_t)); false when it would pass the last address
static inline bool stage_span_end(const void *base, size_t slots, size_t stride, uintptr_t *end)
{
    const uintptr_t b = (uintptr_t)base, room = (UINTPTR_MAX - b) / sizeof(int16_t);
    if (slots != 0 && stride > room / slots)
        return false;
    *end = b + (uintptr_t)slots * stride * sizeof(int16_t);
    return true;
}

static inline StageRunError stage_run_check(const StageRun &r, size_t *where)
{
    if (!r.in || !r.out)
        return STAGE_RUN_NULL;
    if (((uintptr_t)r.in | (uintptr_t)r.out) & 15u)
        return STAGE_RUN_ALIGN;
    if ((r.in_stride | r.out_stride) & 7u)
        return STAGE_RUN_STRIDE8;
    if (r.frames > r.max_frames)
        return STAGE_RUN_FRAMES;
    if (r.counts)
        for (size_t s = 0; s < r.in_slots; s++)
            if (r.counts[s] > r.frames) {
                if (where)
                    *where = s;
                return STAGE_RUN_COUNT;
            }
    // (stride < frames * channels, without the product: it may not fit)
    if (r.in_channels && r.in_stride / r.in_channels < r.frames)
        return STAGE_RUN_IN_STRIDE;
    if (r.out_channels && r.out_stride / r.out_channels < r.out_frames)
        return STAGE_RUN_OUT_STRIDE;
    uintptr_t ie, oe;
    if (!stage_span_end(r.in, r.in_slots, r.in_stride, &ie) || !stage_span_end(r.out, r.out_slots, r.out_stride, &oe))
        return STAGE_RUN_SPAN;
    const uintptr_t ib = (uintptr_t)r.in, ob = (uintptr_t)r.out;
    if (r.overlap == STAGE_APART ? (ib < oe && ob < ie) : ib == ob)
        return STAGE_RUN_OVERLAP;
    return STAGE_RUN_OK;
}

}  // namespace cmhip
#endif
