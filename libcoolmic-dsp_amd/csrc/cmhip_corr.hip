// cmhip_corr.hip -- the phase-correlation / balance meter of a batch on the host side: the opt-in state, the channel
// pairs, the launch of k_corr.hip's kernel ahead of a run's block kernel, the windows' results with the finish in
// double.
//
// Device state (made on the first cmhip_batch_set_correlation(b, 1)): the windows, 64-bit [S][8][3] sums of x_a^2,
// x_b^2 and x_a * x_b per stream and pair.  No filter, no history, no parity slot.  The frames a window accounts are
// counted on the host, where every run's counts are known.  The VU, true-peak and loudness windows know nothing of
// this.  The windows' lifecycle is the shared one of csrc/cmhip_meter.h.
#include "cmhip_engine.h"

#include <math.h>
#include <string.h>

#include <atomic>

// test hook: correlation passes launched by this process so far
static std::atomic<unsigned long long> g_corr_runs{0};
extern "C" unsigned long long cmhip_debug_corr_count(void) { return g_corr_runs.load(); }

static_assert(CORR_MAX_PAIRS == CMHIP_CORR_MAX_PAIRS, "the public limit is the kernels'");

extern "C" double cmhip_corr_value(uint64_t energy_a, uint64_t energy_b, int64_t cross)
{
    if (energy_a == 0 || energy_b == 0)
        return 0.0;
    const double v = (double)cross / sqrt((double)energy_a * (double)energy_b);
    return v > 1.0 ? 1.0 : v < -1.0 ? -1.0 : v;
}

extern "C" double cmhip_corr_balance_db(uint64_t energy_a, uint64_t energy_b)
{
    if (energy_a == 0 && energy_b == 0)
        return 0.0;
    return 10.0 * log10((double)energy_a / (double)energy_b);
}

extern "C" int cmhip_batch_corr_set_pairs(cmhip_batch_t *b, unsigned int n, const unsigned char pairs[][2])
{
    if (!b || !pairs)
        return fail(COOLMIC_ERROR_FAULT, "corr_set_pairs: NULL argument");
    if (n == 0 || n > CORR_MAX_PAIRS)
        return fail(COOLMIC_ERROR_INVAL, "corr_set_pairs: 1 to %u pairs", CORR_MAX_PAIRS);
    for (unsigned i = 0; i < n; i++)
        if (pairs[i][0] == pairs[i][1] || pairs[i][0] >= b->d.channels || pairs[i][1] >= b->d.channels)
            return fail(COOLMIC_ERROR_INVAL, "corr_set_pairs: pair %u (%u, %u) of a batch of %u channels", i,
                        pairs[i][0], pairs[i][1], b->d.channels);
    if (!b->corr.windows_empty())
        return fail(COOLMIC_ERROR_BUSY, "corr_set_pairs: a window holds frames (result or reset first)");
    b->corr_npairs = n;
    for (unsigned i = 0; i < n; i++) {
        b->corr_a[i] = pairs[i][0];
        b->corr_b[i] = pairs[i][1];
    }
    return COOLMIC_ERROR_NONE;
}

int cmhip_engine_corr_run(cmhip_batch_t *b, const int16_t *in, size_t frames, const uint32_t *frames_per_stream)
{
    CorrArgs a;
    memset(&a, 0, sizeof(a));
    a.in = in;
    a.param = b->d_param;
    a.nframes = frames_per_stream ? b->d_nframes : nullptr;
    a.sums = b->corr.windows<unsigned long long>();
    a.frames = (uint32_t)frames;
    a.streams = b->d.streams;
    a.channels = b->d.channels;
    a.npairs = b->corr_npairs;
    memcpy(a.a, b->corr_a, sizeof(a.a));
    memcpy(a.b, b->corr_b, sizeof(a.b));
    a.stride = b->stride;
    const hipError_t e = launch_corr(a, b->stream);
    if (e != hipSuccess)
        return fail(COOLMIC_ERROR_GENERIC, "run: the correlation pass: %s", hipGetErrorString(e));
    g_corr_runs.fetch_add(1, std::memory_order_relaxed);
    b->corr.account(frames, frames_per_stream);
    return COOLMIC_ERROR_NONE;
}

// one window's result from its sums; out is left alone while the window holds no frame
static int corr_finish(const cmhip_batch_t *b, size_t s, const void *window, const void *, void *result)
{
    const unsigned long long frames = b->corr.frames[s];
    if (frames == 0)
        return COOLMIC_ERROR_INVAL;
    const unsigned long long *const sums = (const unsigned long long *)window;
    coolmic_correlation_result_t *const out = (coolmic_correlation_result_t *)result;
    // the stereo kernel sums channel 0, channel 1 and their product whichever way round the one pair names them
    const bool swapped = b->d.channels == 2 && b->corr_npairs == 1 && b->corr_a[0] == 1;
    memset(out, 0, sizeof(*out));
    out->rate = b->d.rate;
    out->channels = b->d.channels;
    out->frames = (size_t)frames;
    out->pairs = b->corr_npairs;
    for (unsigned i = 0; i < b->corr_npairs; i++) {
        const unsigned long long *w = sums + i * CORR_SUMS;
        out->a[i] = b->corr_a[i];
        out->b[i] = b->corr_b[i];
        out->energy_a[i] = swapped ? w[1] : w[0];
        out->energy_b[i] = swapped ? w[0] : w[1];
        out->cross[i] = (int64_t)w[2];
        out->correlation[i] = cmhip_corr_value(out->energy_a[i], out->energy_b[i], out->cross[i]);
        out->balance_db[i] = cmhip_corr_balance_db(out->energy_a[i], out->energy_b[i]);
    }
    return COOLMIC_ERROR_NONE;
}

static const MeterKind CORR = {"corr", "correlation", "correlation", &cmhip_batch::corr,
                               sizeof(coolmic_correlation_result_t), corr_finish, nullptr};

extern "C" int cmhip_batch_set_correlation(cmhip_batch_t *b, int on)
{
    if (b && on && b->d.channels < 2)
        return fail(COOLMIC_ERROR_INVAL, "set_correlation: a mono batch has no channel pair");
    return cmhip_meter_switch(b, CORR, on);  // (the pairs stay across off and on)
}

extern "C" int cmhip_batch_get_correlation(const cmhip_batch_t *b) { return cmhip_meter_get(b, CORR); }

extern "C" int cmhip_batch_corr_result(cmhip_batch_t *b, unsigned int stream, coolmic_correlation_result_t *out)
{
    return cmhip_meter_fetch_one(b, CORR, stream, out);
}

extern "C" int cmhip_batch_corr_results(cmhip_batch_t *b, coolmic_correlation_result_t *out, int *rc)
{
    return cmhip_meter_fetch_all(b, CORR, out, rc);
}

extern "C" int cmhip_batch_corr_reset(cmhip_batch_t *b, long stream)
{
    return cmhip_meter_clear_range(b, CORR, stream);
}
