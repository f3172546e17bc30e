// cmhip_watch.hip -- the signal watch of a batch on the host side: the opt-in state, the thresholds, the launch of
// k_watch.hip's two kernels ahead of a run's block kernel, the windows' results with the DC finish in double.
//
// Device state (made on the first cmhip_batch_set_watch(b, 1)): one array of 64-bit words, the windows
// [S][WATCH_WINDOW_WORDS] (frames, longest run and events per predicate, the channel sums) and behind them the state
// [S][WATCH_SLOTS], the run lengths the streams brought along (csrc/watch_plan.h); and a scratch array of tile
// summaries sized by the launch plan and grown on need.  The frames a window accounts are counted on the host, where
// every run's counts are known.  The windows' lifecycle is the shared one of csrc/cmhip_meter.h, the state its
// state_bytes.
#include "cmhip_engine.h"

#include <math.h>
#include <string.h>

#include <atomic>

// test hook: watch passes launched by this process so far
static std::atomic<unsigned long long> g_watch_runs{0};
extern "C" unsigned long long cmhip_debug_watch_count(void) { return g_watch_runs.load(); }

static_assert(WATCH_MAX_CH == COOLMIC_DSP_VUMETER_MAX_CHANNELS, "the result's arrays are the kernels'");
static_assert(sizeof(coolmic_watch_result_t) == 1080, "the size the header states");

constexpr size_t WORD = sizeof(unsigned long long);

extern "C" unsigned int cmhip_watch_level(double db)
{
    const double v = 32768.0 * pow(10.0, db / 20.0);
    if (!(v > 0.0))                              // (-inf, and NaN)
        return 0;
    if (v >= 32767.0)
        return 32767;
    return (unsigned int)lround(v);
}

extern "C" int cmhip_batch_watch_configure(cmhip_batch_t *b, unsigned int quiet, unsigned int rail, unsigned int clip_run)
{
    if (!b)
        return fail(COOLMIC_ERROR_FAULT, "watch_configure: batch is NULL");
    if (quiet > 32767 || rail < 1 || rail > 32767 || clip_run < 1 || clip_run > WATCH_MAX_RUN)
        return fail(COOLMIC_ERROR_INVAL, "watch_configure: quiet 0..32767, rail 1..32767, clip_run 1..%u (got %u, %u, %u)",
                    WATCH_MAX_RUN, quiet, rail, clip_run);
    if (!b->watch.windows_empty())
        return fail(COOLMIC_ERROR_BUSY, "watch_configure: a window holds frames (result or reset first)");
    if (b->watch.on) {                       // the predicates change: no run continues across that
        if (use(b))
            return COOLMIC_ERROR_GENERIC;
        HIP_TRY(hipMemsetAsync(b->watch.d, 0, (size_t)b->d.streams * WATCH_WORDS * WORD, b->stream));
    }
    b->watch_quiet = quiet;
    b->watch_rail = rail;
    b->watch_run = clip_run;
    return COOLMIC_ERROR_NONE;
}

static int watch_launch(cmhip_batch_t *b, const int16_t *in, size_t frames, const uint32_t *frames_per_stream,
                        hipEvent_t *ev)
{
    const WatchPlan p = watch_plan(b->d.streams, b->d.channels, (uint32_t)frames);
    if (p.refused)
        return fail(COOLMIC_ERROR_GENERIC, "run: the watch pass: the grid would reach 2^31 workgroups");
    if (p.scratch > b->watch_scratch_n) {    // (hipFree waits for what still reads the old array)
        (void)hipFree(b->d_watch_scratch);
        b->d_watch_scratch = nullptr;
        b->watch_scratch_n = 0;
        HIP_TRY(hipMalloc((void **)&b->d_watch_scratch, p.scratch * sizeof(WatchSum)));
        b->watch_scratch_n = p.scratch;
    }
    WatchArgs a;
    memset(&a, 0, sizeof(a));
    a.in = in;
    a.param = b->d_param;
    a.nframes = frames_per_stream ? b->d_nframes : nullptr;
    a.words = b->watch.windows<unsigned long long>();
    a.state = b->watch.state<unsigned long long>(b->d.streams);
    a.scratch = b->d_watch_scratch;
    a.frames = (uint32_t)frames;
    a.streams = b->d.streams;
    a.channels = b->d.channels;
    a.quiet = b->watch_quiet;
    a.rail = b->watch_rail;
    a.clip_run = b->watch_run;
    a.stride = b->stride;
    const hipError_t e = launch_watch(a, p, b->stream, ev);
    if (e != hipSuccess)
        return fail(COOLMIC_ERROR_GENERIC, "run: the watch pass: %s", hipGetErrorString(e));
    g_watch_runs.fetch_add(1, std::memory_order_relaxed);
    b->watch.account(frames, frames_per_stream);
    return COOLMIC_ERROR_NONE;
}

int cmhip_engine_watch_run(cmhip_batch_t *b, const int16_t *in, size_t frames, const uint32_t *frames_per_stream)
{
    return watch_launch(b, in, frames, frames_per_stream, nullptr);
}

// measurement hook (tools/bench_watch.py): the watch's two kernels alone over the batch's own input slots, `frames`
// frames of every stream, with events around each: ms[0] the tile pass, ms[1] the fold.  The frames are accounted as a
// run's are.  The batch has the watch on and slots of its own.
extern "C" int cmhip_test_watch_time(cmhip_batch_t *b, size_t frames, float ms[2])
{
    if (!b || !ms)
        return fail(COOLMIC_ERROR_FAULT, "watch_time: NULL argument");
    if (!b->watch.on || !b->d_in || frames == 0 || frames > b->d.max_frames)
        return fail(COOLMIC_ERROR_INVAL, "watch_time: a batch with the watch on and slots of its own, 1..max_frames frames");
    if (use(b) || cmhip_engine_flush_params(b))
        return COOLMIC_ERROR_GENERIC;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    int rc = COOLMIC_ERROR_GENERIC;
    if (hipEventCreate(&ev[0]) == hipSuccess && hipEventCreate(&ev[1]) == hipSuccess &&
        hipEventCreate(&ev[2]) == hipSuccess && watch_launch(b, b->d_in, frames, nullptr, ev) == COOLMIC_ERROR_NONE &&
        hipEventSynchronize(ev[2]) == hipSuccess && hipEventElapsedTime(&ms[0], ev[0], ev[1]) == hipSuccess &&
        hipEventElapsedTime(&ms[1], ev[1], ev[2]) == hipSuccess)
        rc = COOLMIC_ERROR_NONE;
    for (hipEvent_t e : ev)
        if (e)
            (void)hipEventDestroy(e);
    return rc;
}

// one window's result from its words and the stream's state; out is left alone while the window holds no frame
static int watch_finish(const cmhip_batch_t *b, size_t s, const void *window, const void *state, void *result)
{
    const unsigned long long frames = b->watch.frames[s];
    if (frames == 0)
        return COOLMIC_ERROR_INVAL;
    const unsigned long long *const w = (const unsigned long long *)window, *const st = (const unsigned long long *)state;
    coolmic_watch_result_t *const out = (coolmic_watch_result_t *)result;
    const unsigned C = b->d.channels;
    memset(out, 0, sizeof(*out));
    out->rate = b->d.rate;
    out->channels = C;
    out->frames = (size_t)frames;
    out->quiet = b->watch_quiet;
    out->rail = b->watch_rail;
    out->clip_run = b->watch_run;
    // (the window holds a frame, so the state is the run length at the window's last frame)
    out->dead_frames = w[WATCH_W_CNT];
    out->dead_longest = w[WATCH_W_LONGEST];
    out->dead_current = st[0];
    for (unsigned c = 0; c < C; c++) {
        const unsigned q = 1 + c, r = 1 + WATCH_MAX_CH + c;
        out->quiet_frames[c] = w[WATCH_W_CNT + q];
        out->quiet_longest[c] = w[WATCH_W_LONGEST + q];
        out->quiet_current[c] = st[q];
        out->clip_samples[c] = w[WATCH_W_CNT + r];
        out->clip_longest[c] = w[WATCH_W_LONGEST + r];
        out->clip_events[c] = w[WATCH_W_EV + r];
        out->sum[c] = (int64_t)w[WATCH_W_SUM + c];
        out->dc[c] = (double)out->sum[c] / (double)frames / 32768.0;
    }
    return COOLMIC_ERROR_NONE;
}

// (a result clears the window and keeps the state; on, reset and a configure while on clear both)
static const MeterKind WATCH = {"watch", "watch", "the watch", &cmhip_batch::watch, sizeof(coolmic_watch_result_t),
                                watch_finish, nullptr};

extern "C" int cmhip_batch_set_watch(cmhip_batch_t *b, int on) { return cmhip_meter_switch(b, WATCH, on); }
extern "C" int cmhip_batch_get_watch(const cmhip_batch_t *b) { return cmhip_meter_get(b, WATCH); }

extern "C" int cmhip_batch_watch_result(cmhip_batch_t *b, unsigned int stream, coolmic_watch_result_t *out)
{
    return cmhip_meter_fetch_one(b, WATCH, stream, out);
}

extern "C" int cmhip_batch_watch_results(cmhip_batch_t *b, coolmic_watch_result_t *out, int *rc)
{
    return cmhip_meter_fetch_all(b, WATCH, out, rc);
}

extern "C" int cmhip_batch_watch_reset(cmhip_batch_t *b, long stream) { return cmhip_meter_clear_range(b, WATCH, stream); }

