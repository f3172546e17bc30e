// cmhip_corr.hip -- the phase-correlation / balance meter of a batch on the host side: the opt-in state, the channel
// pairs, the launch of k_corr.hip's kernel ahead of a run's block kernel, the windows' results with the finish in
// double.
//
// Device state (made on the first cmhip_batch_set_correlation(b, 1)): the windows, 64-bit [S][8][3] sums of x_a^2,
// x_b^2 and x_a * x_b per stream and pair.  No filter, no history, no parity slot.  The frames a window accounts are
// counted on the host, where every run's counts are known.  The VU, true-peak and loudness windows know nothing of
// this.
#include "cmhip_engine.h"

#include <math.h>
#include <string.h>

#include <atomic>

// test hook: correlation passes launched by this process so far
static std::atomic<unsigned long long> g_corr_runs{0};
extern "C" unsigned long long cmhip_debug_corr_count(void) { return g_corr_runs.load(); }

constexpr size_t CORR_WORDS = CORR_MAX_PAIRS * CORR_SUMS;    // 64-bit words per stream
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

static bool corr_windows_empty(const cmhip_batch_t *b)
{
    if (!b->corr_on)
        return true;
    for (unsigned long long f : b->corr_frames)
        if (f)
            return false;
    return true;
}

extern "C" int cmhip_batch_set_correlation(cmhip_batch_t *b, int on)
{
    if (!b)
        return fail(COOLMIC_ERROR_FAULT, "set_correlation: batch is NULL");
    if (on && b->d.channels < 2)
        return fail(COOLMIC_ERROR_INVAL, "set_correlation: a mono batch has no channel pair");
    if (on && b->nsec)
        return fail(COOLMIC_ERROR_INVAL, "set_correlation: the equaliser has sections, and correlation does not measure its result");
    if (use(b))
        return COOLMIC_ERROR_GENERIC;
    HIP_TRY(hipStreamSynchronize(b->stream));
    if (!on) {
        b->corr_on = false;                  // (the windows are cleared when it is turned on again; the pairs stay)
        return COOLMIC_ERROR_NONE;
    }
    if (b->corr_on)
        return COOLMIC_ERROR_NONE;
    const size_t S = b->d.streams;
    if (!b->d_corr) {
        HIP_TRY(hipMalloc((void **)&b->d_corr, S * CORR_WORDS * sizeof(unsigned long long)));
        b->corr_host.assign(S * CORR_WORDS, 0);
    }
    HIP_TRY(hipMemsetAsync(b->d_corr, 0, S * CORR_WORDS * sizeof(unsigned long long), b->stream));
    b->corr_frames.assign(S, 0);
    b->corr_on = true;
    return COOLMIC_ERROR_NONE;
}

extern "C" int cmhip_batch_get_correlation(const cmhip_batch_t *b)
{
    if (!b)
        return fail(COOLMIC_ERROR_FAULT, "get_correlation: batch is NULL");
    return b->corr_on ? 1 : 0;
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
    if (!corr_windows_empty(b))
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
    a.sums = b->d_corr;
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
    for (unsigned s = 0; s < b->d.streams; s++)
        b->corr_frames[s] += frames_per_stream ? frames_per_stream[s] : frames;
    return COOLMIC_ERROR_NONE;
}

// one window's result from its sums; out is left alone while the window holds no frame
static int corr_finish(const cmhip_batch_t *b, unsigned long long frames, const unsigned long long *sums,
                       coolmic_correlation_result_t *out)
{
    if (frames == 0)
        return COOLMIC_ERROR_INVAL;
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

extern "C" int cmhip_batch_corr_result(cmhip_batch_t *b, unsigned int stream, coolmic_correlation_result_t *out)
{
    if (!b || !out)
        return fail(COOLMIC_ERROR_FAULT, "corr_result: NULL argument");
    if (!b->corr_on || stream >= b->d.streams)
        return fail(COOLMIC_ERROR_INVAL, "corr_result: stream out of range or batch without correlation");
    if (b->corr_frames[stream] == 0)
        return fail(COOLMIC_ERROR_INVAL, "corr_result: the window holds no frame");
    if (use(b))
        return COOLMIC_ERROR_GENERIC;
    unsigned long long sums[CORR_WORDS];
    unsigned long long *const window = b->d_corr + (size_t)stream * CORR_WORDS;
    HIP_TRY(hipMemcpyAsync(sums, window, sizeof(sums), hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    const int rc = corr_finish(b, b->corr_frames[stream], sums, out);
    HIP_TRY(hipMemsetAsync(window, 0, sizeof(sums), b->stream));
    b->corr_frames[stream] = 0;
    return rc;
}

extern "C" int cmhip_batch_corr_results(cmhip_batch_t *b, coolmic_correlation_result_t *out, int *rc)
{
    if (!b || !out)
        return fail(COOLMIC_ERROR_FAULT, "corr_results: NULL argument");
    if (!b->corr_on)
        return fail(COOLMIC_ERROR_INVAL, "corr_results: batch without correlation");
    if (use(b))
        return COOLMIC_ERROR_GENERIC;
    // one round trip for all streams: behind what the stream has queued, read the windows, clear them on the stream
    const size_t S = b->d.streams, bytes = S * CORR_WORDS * sizeof(unsigned long long);
    HIP_TRY(hipMemcpyAsync(b->corr_host.data(), b->d_corr, bytes, hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    HIP_TRY(hipMemsetAsync(b->d_corr, 0, bytes, b->stream));
    for (size_t s = 0; s < S; s++) {
        const int r = corr_finish(b, b->corr_frames[s], &b->corr_host[s * CORR_WORDS], &out[s]);
        if (rc)
            rc[s] = r;
        b->corr_frames[s] = 0;
    }
    return COOLMIC_ERROR_NONE;
}

extern "C" int cmhip_batch_corr_reset(cmhip_batch_t *b, long stream)
{
    if (!b)
        return fail(COOLMIC_ERROR_FAULT, "corr_reset: batch is NULL");
    const StreamRange sr = stream_range(stream, b->d.streams);
    if (!b->corr_on || !sr.ok)
        return fail(COOLMIC_ERROR_INVAL, "corr_reset: stream %ld out of range or batch without correlation", stream);
    if (use(b))
        return COOLMIC_ERROR_GENERIC;
    const size_t lo = sr.lo, n = sr.n;
    HIP_TRY(hipMemsetAsync(b->d_corr + lo * CORR_WORDS, 0, n * CORR_WORDS * sizeof(unsigned long long), b->stream));
    for (size_t s = lo; s < lo + n; s++)
        b->corr_frames[s] = 0;
    return COOLMIC_ERROR_NONE;
}
