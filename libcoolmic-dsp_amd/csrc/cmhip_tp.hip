// cmhip_tp.hip -- true peak (ITU-R BS.1770 Annex 2 / EBU R128) of a batch on the host side: the opt-in state, the
// launch of k_tpeak.hip's kernel ahead of a run's block kernel, the windows' results with the dBTP finish in double.
//
// Device state (made on the first cmhip_batch_set_true_peak(b, 1)): the windows, uint32 [S][16] maxima of |y|, and
// the streams' filter history, int16 [2][S][16][11], two slots selected by a parity the host flips per run (the
// mechanism of VuState::samples).  The frames a window accounts are counted on the host, where every run's counts
// are known.  The VU windows, their snapshots and records know nothing of this.
#include "cmhip_engine.h"

#include <math.h>
#include <string.h>

#include <atomic>

// test hook: true-peak passes launched by this process so far
static std::atomic<unsigned long long> g_tp_runs{0};
extern "C" unsigned long long cmhip_debug_tp_count(void) { return g_tp_runs.load(); }

static size_t tp_hist_words(const cmhip_batch_t *b) { return (size_t)b->d.streams * MAX_CH * TP_HIST; }

extern "C" double cmhip_tp_dbtp(uint32_t peak)
{
    return 20. * log10((double)peak / 268435456.);
}

extern "C" void cmhip_tp_coefficients(int16_t h[48])
{
    if (!h)
        return;
    for (unsigned p = 0; p < 4; p++)
        for (unsigned k = 0; k < TP_TAPS; k++)
            h[p * TP_TAPS + k] = tp_h(p, k);
}

extern "C" int cmhip_batch_set_true_peak(cmhip_batch_t *b, int on)
{
    if (!b)
        return fail(COOLMIC_ERROR_FAULT, "set_true_peak: batch is NULL");
    if (on && b->nsec)
        return fail(COOLMIC_ERROR_INVAL, "set_true_peak: the equaliser has sections, and true peak does not measure its result");
    if (use(b))
        return COOLMIC_ERROR_GENERIC;
    HIP_TRY(hipStreamSynchronize(b->stream));
    if (!on) {
        b->tp_on = false;                    // (windows and history are cleared when it is turned on again)
        return COOLMIC_ERROR_NONE;
    }
    if (b->tp_on)
        return COOLMIC_ERROR_NONE;
    const size_t S = b->d.streams;
    if (!b->d_tp_peak) {
        HIP_TRY(hipMalloc((void **)&b->d_tp_peak, S * MAX_CH * sizeof(uint32_t)));
        HIP_TRY(hipMalloc((void **)&b->d_tp_hist, 2 * tp_hist_words(b) * sizeof(int16_t)));
        b->tp_host.assign(S * MAX_CH, 0);
    }
    HIP_TRY(hipMemsetAsync(b->d_tp_peak, 0, S * MAX_CH * sizeof(uint32_t), b->stream));
    HIP_TRY(hipMemsetAsync(b->d_tp_hist, 0, 2 * tp_hist_words(b) * sizeof(int16_t), b->stream));
    b->tp_frames.assign(S, 0);
    b->tp_parity = 0;
    b->tp_on = true;
    return COOLMIC_ERROR_NONE;
}

extern "C" int cmhip_batch_get_true_peak(const cmhip_batch_t *b)
{
    if (!b)
        return fail(COOLMIC_ERROR_FAULT, "get_true_peak: batch is NULL");
    return b->tp_on ? 1 : 0;
}

int cmhip_engine_tp_run(cmhip_batch_t *b, const int16_t *in, size_t frames, const uint32_t *frames_per_stream)
{
    TpArgs a;
    memset(&a, 0, sizeof(a));
    a.in = in;
    a.param = b->d_param;
    a.nframes = frames_per_stream ? b->d_nframes : nullptr;
    a.peak = b->d_tp_peak;
    a.hist = b->d_tp_hist;
    a.frames = (uint32_t)frames;
    a.streams = b->d.streams;
    a.channels = b->d.channels;
    a.parity = b->tp_parity;
    a.stride = b->stride;
    const hipError_t e = launch_tpeak(a, b->stream);
    if (e != hipSuccess)
        return fail(COOLMIC_ERROR_GENERIC, "run: the true-peak pass: %s", hipGetErrorString(e));
    g_tp_runs.fetch_add(1, std::memory_order_relaxed);
    b->tp_parity ^= 1u;                      // the kernel wrote the other history slot
    for (unsigned s = 0; s < b->d.streams; s++)
        b->tp_frames[s] += frames_per_stream ? frames_per_stream[s] : frames;
    return COOLMIC_ERROR_NONE;
}

// one window's result from its maxima; out is left alone while the window holds no frame
static int tp_finish(const cmhip_batch_t *b, unsigned long long frames, const uint32_t *peak,
                     coolmic_truepeak_result_t *out)
{
    if (frames == 0)
        return COOLMIC_ERROR_INVAL;
    const unsigned C = b->d.channels;
    memset(out, 0, sizeof(*out));
    out->rate = b->d.rate;
    out->channels = C;
    out->frames = (size_t)frames;
    uint32_t all = 0;
    for (unsigned c = 0; c < C; c++) {
        out->channel_peak[c] = peak[c];
        out->channel_dbtp[c] = cmhip_tp_dbtp(peak[c]);
        if (peak[c] > all)
            all = peak[c];
    }
    out->global_peak = all;
    out->global_dbtp = cmhip_tp_dbtp(all);
    return COOLMIC_ERROR_NONE;
}

extern "C" int cmhip_batch_tp_result(cmhip_batch_t *b, unsigned int stream, coolmic_truepeak_result_t *out)
{
    if (!b || !out)
        return fail(COOLMIC_ERROR_FAULT, "tp_result: NULL argument");
    if (!b->tp_on || stream >= b->d.streams)
        return fail(COOLMIC_ERROR_INVAL, "tp_result: stream out of range or batch without true peak");
    if (b->tp_frames[stream] == 0)
        return fail(COOLMIC_ERROR_INVAL, "tp_result: the window holds no frame");
    if (use(b))
        return COOLMIC_ERROR_GENERIC;
    uint32_t peak[MAX_CH];
    uint32_t *const window = b->d_tp_peak + (size_t)stream * MAX_CH;
    HIP_TRY(hipMemcpyAsync(peak, window, sizeof(peak), hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    const int rc = tp_finish(b, b->tp_frames[stream], peak, out);
    HIP_TRY(hipMemsetAsync(window, 0, sizeof(peak), b->stream));
    b->tp_frames[stream] = 0;
    return rc;
}

extern "C" int cmhip_batch_tp_results(cmhip_batch_t *b, coolmic_truepeak_result_t *out, int *rc)
{
    if (!b || !out)
        return fail(COOLMIC_ERROR_FAULT, "tp_results: NULL argument");
    if (!b->tp_on)
        return fail(COOLMIC_ERROR_INVAL, "tp_results: batch without true peak");
    if (use(b))
        return COOLMIC_ERROR_GENERIC;
    // one round trip for all streams: behind what the stream has queued, read the windows, clear them on the stream
    const size_t S = b->d.streams, bytes = S * MAX_CH * sizeof(uint32_t);
    HIP_TRY(hipMemcpyAsync(b->tp_host.data(), b->d_tp_peak, bytes, hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    HIP_TRY(hipMemsetAsync(b->d_tp_peak, 0, bytes, b->stream));
    for (size_t s = 0; s < S; s++) {
        const int r = tp_finish(b, b->tp_frames[s], &b->tp_host[s * MAX_CH], &out[s]);
        if (rc)
            rc[s] = r;
        b->tp_frames[s] = 0;
    }
    return COOLMIC_ERROR_NONE;
}

extern "C" int cmhip_batch_tp_reset(cmhip_batch_t *b, long stream)
{
    if (!b)
        return fail(COOLMIC_ERROR_FAULT, "tp_reset: batch is NULL");
    const StreamRange sr = stream_range(stream, b->d.streams);
    if (!b->tp_on || !sr.ok)
        return fail(COOLMIC_ERROR_INVAL, "tp_reset: stream %ld out of range or batch without true peak", stream);
    if (use(b))
        return COOLMIC_ERROR_GENERIC;
    const size_t lo = sr.lo, n = sr.n;
    HIP_TRY(hipMemsetAsync(b->d_tp_peak + lo * MAX_CH, 0, n * MAX_CH * sizeof(uint32_t), b->stream));
    for (unsigned slot = 0; slot < 2; slot++)
        HIP_TRY(hipMemsetAsync(b->d_tp_hist + slot * tp_hist_words(b) + lo * MAX_CH * TP_HIST, 0,
                               n * MAX_CH * TP_HIST * sizeof(int16_t), b->stream));
    for (size_t s = lo; s < lo + n; s++)
        b->tp_frames[s] = 0;
    return COOLMIC_ERROR_NONE;
}
