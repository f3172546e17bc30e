// cmhip_tp.hip -- true peak (ITU-R BS.1770 Annex 2 / EBU R128) of a batch on the host side: the meter's kind, the
// launch of k_tpeak.hip's kernel ahead of a run's block kernel, the windows' finish with dBTP in double.
//
// Device state (made on the first cmhip_batch_set_true_peak(b, 1)): the windows, uint32 [S][16] maxima of |y|, and
// the streams' filter history, int16 [2][S][16][11], two slots selected by a parity the host flips per run (the
// mechanism of VuState::samples).  The frames a window accounts are counted on the host, where every run's counts
// are known.  The VU windows, their snapshots and records know nothing of this.  The windows' lifecycle is the shared
// one of csrc/cmhip_meter.h.
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

// beside the windows: both history slots, made once and cleared
static int tp_turn_on(cmhip_batch_t *b)
{
    if (!b->d_tp_hist)
        HIP_TRY(hipMalloc((void **)&b->d_tp_hist, 2 * tp_hist_words(b) * sizeof(int16_t)));
    HIP_TRY(hipMemsetAsync(b->d_tp_hist, 0, 2 * tp_hist_words(b) * sizeof(int16_t), b->stream));
    b->tp_parity = 0;
    return COOLMIC_ERROR_NONE;
}

int cmhip_engine_tp_run(cmhip_batch_t *b, const int16_t *in, size_t frames, const uint32_t *frames_per_stream)
{
    TpArgs a;
    memset(&a, 0, sizeof(a));
    a.in = in;
    a.param = b->d_param;
    a.nframes = frames_per_stream ? b->d_nframes : nullptr;
    a.peak = b->tp.windows<uint32_t>();
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
    b->tp.account(frames, frames_per_stream);
    return COOLMIC_ERROR_NONE;
}

// one window's result from its maxima; out is left alone while the window holds no frame
static int tp_finish(const cmhip_batch_t *b, size_t s, const void *window, const void *, void *result)
{
    const unsigned long long frames = b->tp.frames[s];
    if (frames == 0)
        return COOLMIC_ERROR_INVAL;
    const uint32_t *const peak = (const uint32_t *)window;
    coolmic_truepeak_result_t *const out = (coolmic_truepeak_result_t *)result;
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

static const MeterKind TP = {"tp", "true_peak", "true peak", &cmhip_batch::tp, sizeof(coolmic_truepeak_result_t),
                             tp_finish, tp_turn_on};

extern "C" int cmhip_batch_set_true_peak(cmhip_batch_t *b, int on) { return cmhip_meter_switch(b, TP, on); }
extern "C" int cmhip_batch_get_true_peak(const cmhip_batch_t *b) { return cmhip_meter_get(b, TP); }

extern "C" int cmhip_batch_tp_result(cmhip_batch_t *b, unsigned int stream, coolmic_truepeak_result_t *out)
{
    return cmhip_meter_fetch_one(b, TP, stream, out);
}

extern "C" int cmhip_batch_tp_results(cmhip_batch_t *b, coolmic_truepeak_result_t *out, int *rc)
{
    return cmhip_meter_fetch_all(b, TP, out, rc);
}

extern "C" int cmhip_batch_tp_reset(cmhip_batch_t *b, long stream)
{
    size_t lo, n;
    const int rc = cmhip_meter_clear_range(b, TP, stream, &lo, &n);
    if (rc != COOLMIC_ERROR_NONE)
        return rc;
    for (unsigned slot = 0; slot < 2; slot++)
        HIP_TRY(hipMemsetAsync(b->d_tp_hist + slot * tp_hist_words(b) + lo * MAX_CH * TP_HIST, 0,
                               n * MAX_CH * TP_HIST * sizeof(int16_t), b->stream));
    return COOLMIC_ERROR_NONE;
}
