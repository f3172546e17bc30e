// stage_io_test.cpp -- csrc/stage_io.h as a stand-alone program: g++ alone compiles it (the header includes no HIP),
// tests/test_stage_io_host.py runs it plainly and under AddressSanitizer + UBSan.  The addresses are made up: the check
// dereferences nothing but the counts.
//   stage_io_test  ->  "stage io ok: N checks"
#include <limits.h>
#include <stdio.h>

#include "stage_io.h"

using namespace cmhip;

static unsigned long checks = 0;

#define CHECK(c)                                                    \
    do {                                                            \
        checks++;                                                   \
        if (!(c)) {                                                 \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                               \
        }                                                           \
    } while (0)

static const void *at(uintptr_t a) { return (const void *)a; }

// a run of the limiter's or the mixer's kind: S slots on both sides, C channels, `frames` frames each
static StageRun same(uintptr_t in, size_t in_stride, size_t frames, uintptr_t out, size_t out_stride, const uint32_t *counts,
                     size_t S, size_t C, size_t max_frames)
{
    return {at(in), at(out), in_stride, out_stride, frames, max_frames, counts, S, S, C, frames, C, STAGE_APART};
}

// a run of the bus's kind: S input slots of CI channels, B output slots of CO
static StageRun bus(uintptr_t in, size_t in_stride, size_t frames, uintptr_t out, size_t out_stride, const uint32_t *counts)
{
    return {at(in), at(out), in_stride, out_stride, frames, 256, counts, 3, 2, 2, frames, 1, STAGE_APART};
}

// a run of the resampler's kind: the output holds out_frames frames, and only in == out is refused
static StageRun src(uintptr_t in, size_t in_stride, size_t frames, uintptr_t out, size_t out_stride, size_t out_frames)
{
    return {at(in), at(out), in_stride, out_stride, frames, 256, nullptr, 2, 2, 2, out_frames, 2, STAGE_NOT_IN_PLACE};
}

static StageRunError run(const StageRun &r, size_t *where = nullptr) { return stage_run_check(r, where); }

static int test_limiter_refusals()
{
    // tests/test_gpu_lim.py::test_refusals: S 2, C 2, stride 520, 256 frames
    const uintptr_t SRC = 0x10000, DST = 0x20000;
    const size_t st = 520;
    const uint32_t counts[2] = {100, 101};
    auto lim = [&](uintptr_t in, size_t ist, size_t n, uintptr_t out, size_t ost, const uint32_t *c = nullptr) {
        return run(same(in, ist, n, out, ost, c, 2, 2, 256));
    };
    CHECK(lim(SRC, st, 256, DST, st) == STAGE_RUN_OK);
    CHECK(lim(SRC + 2, st, 256, DST, st) == STAGE_RUN_ALIGN);
    CHECK(lim(SRC, st, 256, DST + 8, st) == STAGE_RUN_ALIGN);
    CHECK(lim(SRC, st + 4, 256, DST, st) == STAGE_RUN_STRIDE8);
    CHECK(lim(SRC, st, 256, DST, st - 4) == STAGE_RUN_STRIDE8);
    CHECK(lim(SRC, 504, 256, DST, st) == STAGE_RUN_IN_STRIDE);
    CHECK(lim(SRC, st, 256, DST, 504) == STAGE_RUN_OUT_STRIDE);
    CHECK(lim(SRC, st, 257, DST, st) == STAGE_RUN_FRAMES);
    CHECK(lim(SRC, st, 100, DST, st, counts) == STAGE_RUN_COUNT);
    CHECK(lim(SRC, st, 256, SRC, st) == STAGE_RUN_OVERLAP);                          // in == out
    CHECK(lim(SRC, st, 256, SRC + 16, st) == STAGE_RUN_OVERLAP);                     // out inside in
    CHECK(lim(SRC, st, 256, SRC + 2 * (st + 256), st) == STAGE_RUN_OVERLAP);         // out begins in the last slot of in
    CHECK(lim(DST + 2 * st, st, 256, DST, st) == STAGE_RUN_OVERLAP);                 // in begins inside out
    CHECK(lim(0, st, 256, DST, st) == STAGE_RUN_NULL && lim(SRC, st, 256, 0, st) == STAGE_RUN_NULL);
    return 0;
}

static int test_bus_refusals()
{
    // tests/test_gpu_bus.py::test_refusals: S 3, B 2, CI 2, CO 1, strides 512 and 264, 256 frames
    const uintptr_t SRC = 0x10000, DST = 0x20000;
    const size_t si = 512, so = 264;
    const uint32_t counts[3] = {100, 100, 101};
    CHECK(run(bus(SRC, si, 256, DST, so, nullptr)) == STAGE_RUN_OK);
    CHECK(run(bus(SRC + 2, si, 256, DST, so, nullptr)) == STAGE_RUN_ALIGN);
    CHECK(run(bus(SRC, si, 256, DST + 8, so, nullptr)) == STAGE_RUN_ALIGN);
    CHECK(run(bus(SRC, si + 4, 256, DST, so, nullptr)) == STAGE_RUN_STRIDE8);
    CHECK(run(bus(SRC, si, 256, DST, so - 4, nullptr)) == STAGE_RUN_STRIDE8);
    CHECK(run(bus(SRC, 504, 256, DST, so, nullptr)) == STAGE_RUN_IN_STRIDE);
    CHECK(run(bus(SRC, si, 256, DST, 248, nullptr)) == STAGE_RUN_OUT_STRIDE);
    CHECK(run(bus(SRC, si, 257, DST, so, nullptr)) == STAGE_RUN_FRAMES);
    size_t where = 77;
    CHECK(run(bus(SRC, si, 100, DST, so, counts), &where) == STAGE_RUN_COUNT && where == 2);
    CHECK(run(bus(SRC, si, 256, SRC, so, nullptr)) == STAGE_RUN_OVERLAP);
    CHECK(run(bus(SRC, si, 256, SRC + 16, so, nullptr)) == STAGE_RUN_OVERLAP);
    CHECK(run(bus(SRC, si, 256, SRC + 2 * (2 * si + 256), so, nullptr)) == STAGE_RUN_OVERLAP);
    CHECK(run(bus(DST + 2 * so, si, 256, DST, so, nullptr)) == STAGE_RUN_OVERLAP);
    // the output is B slots long, not S: an input that begins where the second bus slot ends is apart from it
    CHECK(run(bus(DST + 2 * 2 * so, si, 256, DST, so, nullptr)) == STAGE_RUN_OK);
    CHECK(run(bus(DST + 2 * 2 * so - 16, si, 256, DST, so, nullptr)) == STAGE_RUN_OVERLAP);
    return 0;
}

static int test_overlap_edges()
{
    const uintptr_t A = 0x10000;
    const size_t st = 520, bytes = 2 * st * sizeof(int16_t);                          // two slots
    auto lim = [&](uintptr_t in, uintptr_t out, size_t n, size_t stride) {
        return run(same(in, stride, n, out, stride, nullptr, 2, 2, 256));
    };
    CHECK(lim(A, A + bytes, 256, st) == STAGE_RUN_OK);                  // out begins exactly where in's last slot ends
    CHECK(lim(A, A + bytes - 16, 256, st) == STAGE_RUN_OVERLAP);        // ... one vector earlier
    CHECK(lim(A + bytes, A, 256, st) == STAGE_RUN_OK);                  // the same with the two swapped
    CHECK(lim(A + bytes - 16, A, 256, st) == STAGE_RUN_OVERLAP);
    // in == out with frames == 0: the rule judges the arrays' bytes, slots * stride of them, not the run's frames --
    // arrays of no bytes share none, arrays of some do
    CHECK(lim(A, A, 0, 0) == STAGE_RUN_OK);
    CHECK(lim(A, A, 0, st) == STAGE_RUN_OVERLAP);
    return 0;
}

static int test_resampler_rule()
{
    const uintptr_t A = 0x10000, B = 0x20000;
    CHECK(run(src(A, 512, 256, B, 512, 256)) == STAGE_RUN_OK);
    CHECK(run(src(A, 512, 256, A, 512, 256)) == STAGE_RUN_OVERLAP);     // in == out
    CHECK(run(src(A, 512, 256, A + 16, 512, 256)) == STAGE_RUN_OK);     // (documented: nothing else is refused)
    CHECK(run(src(A, 512, 0, A, 512, 0)) == STAGE_RUN_OVERLAP);
    // the output is sized by the number passed in, not by frames * C
    CHECK(run(src(A, 512, 256, B, 264, 130)) == STAGE_RUN_OK);          // 130 * 2 = 260 <= 264 < 256 * 2
    CHECK(run(src(A, 512, 256, B, 256, 130)) == STAGE_RUN_OUT_STRIDE);
    CHECK(run(src(A, 104, 50, B, 512, 256)) == STAGE_RUN_OK);           // an upsampling run: 256 * 2 = 512 > 50 * 2
    CHECK(run(src(A, 104, 50, B, 504, 256)) == STAGE_RUN_OUT_STRIDE);
    CHECK(run(src(A, 96, 50, B, 512, 256)) == STAGE_RUN_IN_STRIDE);
    return 0;
}

static int test_counts()
{
    const uintptr_t A = 0x10000, B = 0x20000;
    uint32_t counts[3] = {100, 100, 100};
    size_t where = 77;
    CHECK(run(same(A, 512, 100, B, 512, counts, 3, 2, 256), &where) == STAGE_RUN_OK && where == 77);
    CHECK(run(same(A, 512, 100, B, 512, nullptr, 3, 2, 256), &where) == STAGE_RUN_OK);
    for (size_t s = 0; s < 3; s++) {
        counts[s] = 101;
        where = 77;
        CHECK(run(same(A, 512, 100, B, 512, counts, 3, 2, 256), &where) == STAGE_RUN_COUNT && where == s);
        CHECK(run(same(A, 512, 100, B, 512, counts, 3, 2, 256)) == STAGE_RUN_COUNT);       // (where may be NULL)
        counts[s] = 0;
    }
    CHECK(run(same(A, 512, 100, B, 512, counts, 3, 2, 256)) == STAGE_RUN_OK);
    return 0;
}

static int test_wrap_around()
{
    const uintptr_t A = 0x10000, B = 0x20000;
    const size_t HALF = (size_t)1 << (sizeof(size_t) * 8 - 1);                        // 2^63: a multiple of 8
    // slots * stride * 2 bytes is 2^64 * slots / 2 = 0 mod 2^64: both ranges would look empty and pass the overlap test
    CHECK(run(same(A, HALF, 0, A, HALF, nullptr, 2, 2, 256)) == STAGE_RUN_SPAN);
    CHECK(run(same(A, HALF, 0, B, 512, nullptr, 2, 2, 256)) == STAGE_RUN_SPAN);
    CHECK(run(same(A, 512, 0, B, HALF, nullptr, 2, 2, 256)) == STAGE_RUN_SPAN);
    CHECK(run(same(A, HALF, 0, B, 512, nullptr, 1, 2, 256)) == STAGE_RUN_SPAN);        // one slot: 2^64 bytes exactly
    CHECK(run(src(A, HALF, 0, B, 512, 0)) == STAGE_RUN_SPAN);                         // under either overlap rule
    // the last array that fits ends at the last address
    const size_t fits = ((UINTPTR_MAX - A) / sizeof(int16_t)) & ~(size_t)7;
    uintptr_t end = 0;
    CHECK(stage_span_end(at(A), 1, fits, &end) && end == A + fits * sizeof(int16_t) && end > A);
    CHECK(!stage_span_end(at(A), 1, fits + 8, &end) && !stage_span_end(at(A), 2, fits / 2 + 8, &end));
    CHECK(stage_span_end(at(A), 0, SIZE_MAX, &end) && end == A);                      // no slots: no bytes
    CHECK(run(same(A, fits, 0, 0x8000, 8, nullptr, 1, 2, 256)) == STAGE_RUN_OK);
    // frames * channels = 2^63 * 2 wraps to 0: the stride is below the true product all the same
    CHECK(run(same(A, 512, HALF, B, 512, nullptr, 2, 2, SIZE_MAX)) == STAGE_RUN_IN_STRIDE);
    CHECK(run(same(A, 512, HALF + 1, B, 512, nullptr, 2, 2, SIZE_MAX)) == STAGE_RUN_IN_STRIDE);    // wraps to 2
    StageRun r = same(A, 512, 256, B, 512, nullptr, 2, 2, 256);
    r.out_frames = HALF;
    CHECK(run(r) == STAGE_RUN_OUT_STRIDE);
    CHECK(run(same(A, SIZE_MAX & ~(size_t)7, SIZE_MAX, B, 512, nullptr, 0, 1, SIZE_MAX)) == STAGE_RUN_IN_STRIDE);
    return 0;
}

static bool fits_long(unsigned long v) { return v <= (unsigned long)LONG_MAX; }

static int test_stream_range()
{
    const unsigned sizes[] = {1, 3, UINT_MAX};
    for (unsigned S : sizes) {
        StreamRange r = stream_range(-1, S);
        CHECK(r.ok && r.lo == 0 && r.n == S);
        r = stream_range(0, S);
        CHECK(r.ok && r.lo == 0 && r.n == 1);
        r = stream_range((long)S - 1, S);
        CHECK(r.ok && r.lo == S - 1 && r.n == 1);
        CHECK(!stream_range(-2, S).ok && !stream_range(LONG_MIN, S).ok);
        if (fits_long(S))                                                             // (a long of 64 bits holds every S)
            CHECK(!stream_range((long)S, S).ok);
        CHECK(!stream_range(LONG_MAX, S).ok || !fits_long(S));
    }
    CHECK(!stream_range(3, 3).ok && !stream_range(1, 1).ok && !stream_range(0, 0).ok && stream_range(-1, 0).n == 0);
    return 0;
}

// the two slots of a history [2][S][per]: a run reads slot `parity`, the flip after it makes that the slot it wrote
static int test_history_slots()
{
    HistorySlots h;
    h.streams = 5;
    CHECK(h.parity == 0 && h.at(0, 7) == 0 && h.at(3, 7) == 21);
    h.flip();
    CHECK(h.parity == 1 && h.at(0, 7) == 35 && h.at(3, 7) == 56 && h.at(4, 1) == 9);   // (per 1: the resampler's positions)
    h.flip();
    CHECK(h.parity == 0 && h.at(4, 7) == 28);
    // the last element of the slot a run reads lies inside [2][S][per] whatever the parity
    for (int i = 0; i < 2; i++, h.flip())
        CHECK(h.at(4, 7) + 7 <= 2 * 5 * 7);
    const uint32_t counts[2] = {3, 0};
    CHECK(stage_count(counts, 0, 9) == 3 && stage_count(counts, 1, 9) == 0 && stage_count(nullptr, 1, 9) == 9);
    return 0;
}

int main(void)
{
    if (test_limiter_refusals() || test_bus_refusals() || test_overlap_edges() || test_resampler_rule() || test_counts() ||
        test_wrap_around() || test_stream_range() || test_history_slots())
        return 1;
    printf("stage io ok: %lu checks\n", checks);
    return 0;
}
