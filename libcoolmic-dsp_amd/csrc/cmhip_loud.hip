// cmhip_loud.hip -- programme loudness (ITU-R BS.1770 / EBU R128) of a batch on the host side: the opt-in state, the
// launch of k_loud.hip's kernel ahead of a run's block kernel, the drain of the device's ring of sub-block sums, and
// the finish in double: momentary, short-term, gated integrated loudness.  The arithmetic is specified to the bit in
// include/coolmic_hip.h.
//
// Device state (made on the first cmhip_batch_set_loudness(b, 1)): LoudState [S][C], the rows' filter history and
// open sub-block, and the ring double [S][R][C] of completed sums.  The host knows every run's frame counts, so it
// knows how many sub-blocks each stream has completed without asking the device: it drains the ring before a run that
// could push a stream's undrained count past R and at every result call, and keeps z_j per stream until reset.
#include "cmhip_engine.h"

#include <math.h>
#include <string.h>

#include <atomic>
#include <new>

// test hook: loudness passes launched by this process so far
static std::atomic<unsigned long long> g_loud_runs{0};
extern "C" unsigned long long cmhip_debug_loud_count(void) { return g_loud_runs.load(); }

constexpr size_t LOUD_RECENT = 30;               // sub-blocks whose per-channel sums the host keeps (short-term's span)

// ---------------------------------------------------------------------------
// host only: coefficients, LUFS, gating

extern "C" void cmhip_loud_coefficients(unsigned int rate, double c[10])
{
    if (!c)
        return;
    {
        const double f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196;
        const double K = tan(M_PI * f0 / rate);
        const double Vh = pow(10.0, G / 20.0);
        const double Vb = pow(Vh, 0.4996667741545416);
        const double a0 = 1.0 + K / Q + K * K;
        c[0] = (Vh + Vb * K / Q + K * K) / a0;
        c[1] = 2.0 * (K * K - Vh) / a0;
        c[2] = (Vh - Vb * K / Q + K * K) / a0;
        c[3] = 2.0 * (K * K - 1.0) / a0;
        c[4] = (1.0 - K / Q + K * K) / a0;
    }
    {
        const double f0 = 38.13547087602444, Q = 0.5003270373238773;
        const double K = tan(M_PI * f0 / rate);
        const double a0 = 1.0 + K / Q + K * K;
        c[5] = 1.0;
        c[6] = -2.0;
        c[7] = 1.0;
        c[8] = 2.0 * (K * K - 1.0) / a0;
        c[9] = (1.0 - K / Q + K * K) / a0;
    }
}

extern "C" double cmhip_loud_lufs(double mean_square)
{
    if (mean_square == 0.0)
        return -INFINITY;
    return -0.691 + 10.0 * log10(mean_square);
}

static inline double loud_block(const double *z, size_t i)   // the 400 ms block that ends with sub-block i >= 3
{
    return (((z[i - 3] + z[i - 2]) + z[i - 1]) + z[i]) * 0.25;
}

extern "C" int cmhip_loud_integrate(const double *z, size_t n, double *integrated, double *threshold, size_t *gated)
{
    if (n && !z)
        return fail(COOLMIC_ERROR_FAULT, "loud_integrate: z is NULL");
    double result = -INFINITY, thr = -INFINITY;
    size_t kept = 0;
    if (n >= 4) {
        double sum = 0.0;
        size_t cnt = 0;
        for (size_t i = 3; i < n; i++) {
            const double B = loud_block(z, i);
            if (cmhip_loud_lufs(B) > -70.0) {
                sum += B;
                cnt++;
            }
        }
        if (cnt) {
            thr = cmhip_loud_lufs(sum / (double)cnt) - 10.0;
            sum = 0.0;
            cnt = 0;
            for (size_t i = 3; i < n; i++) {
                const double B = loud_block(z, i);
                const double l = cmhip_loud_lufs(B);
                if (l > -70.0 && l > thr) {
                    sum += B;
                    cnt++;
                }
            }
            if (cnt) {
                result = cmhip_loud_lufs(sum / (double)cnt);
                kept = cnt;
            }
        }
    }
    if (integrated)
        *integrated = result;
    if (threshold)
        *threshold = thr;
    if (gated)
        *gated = kept;
    return COOLMIC_ERROR_NONE;
}

// ---------------------------------------------------------------------------
// the batch

static void loud_clear_host(cmhip_batch_t *b, size_t lo, size_t n)
{
    const size_t C = b->d.channels;
    for (size_t s = lo; s < lo + n; s++) {
        b->loud_frames[s] = 0;
        b->loud_drained[s] = 0;
        b->loud_z[s].clear();
        for (size_t i = 0; i < LOUD_RECENT * C; i++)
            b->loud_recent[s * LOUD_RECENT * C + i] = 0.0;
    }
}

extern "C" int cmhip_batch_set_loudness(cmhip_batch_t *b, int on)
{
    if (!b)
        return fail(COOLMIC_ERROR_FAULT, "set_loudness: batch is NULL");
    if (on && b->nsec)
        return fail(COOLMIC_ERROR_INVAL, "set_loudness: the equaliser has sections, and loudness does not measure its result");
    if (on && (b->d.rate < 8000 || b->d.rate > 384000))
        return fail(COOLMIC_ERROR_INVAL, "set_loudness: rate %u outside 8000..384000", (unsigned)b->d.rate);
    if (use(b))
        return COOLMIC_ERROR_GENERIC;
    HIP_TRY(hipStreamSynchronize(b->stream));
    if (!on) {
        b->loud_on = false;                  // (everything is cleared when it is turned on again)
        return COOLMIC_ERROR_NONE;
    }
    if (b->loud_on)
        return COOLMIC_ERROR_NONE;
    const size_t S = b->d.streams, C = b->d.channels;
    if (!b->d_loud) {
        const unsigned int L = (b->d.rate + 5) / 10;
        const size_t per_run = (b->d.max_frames + L - 1) / L + 1;    // sub-blocks a run can complete, and one
        const size_t R = 4 * per_run > 32 ? 4 * per_run : 32;
        if (R > 0xffffffffu)
            return fail(COOLMIC_ERROR_INVAL, "set_loudness: max_frames too large for a ring");
        try {
            b->loud_w.assign(S * C, 1.0);
            b->loud_frames.assign(S, 0);
            b->loud_drained.assign(S, 0);
            b->loud_z.assign(S, std::vector<double>());
            b->loud_recent.assign(S * LOUD_RECENT * C, 0.0);
            b->loud_host.assign(S * R * C, 0.0);
        } catch (const std::bad_alloc &) {       // (nothing C++ leaves through the C interface)
            return fail(COOLMIC_ERROR_NOMEM, "set_loudness: out of host memory");
        }
        LoudState *st = nullptr;
        double *ring = nullptr;
        if (hipMalloc((void **)&st, S * C * sizeof(LoudState)) != hipSuccess ||
            hipMalloc((void **)&ring, S * R * C * sizeof(double)) != hipSuccess) {
            (void)hipGetLastError();
            (void)hipFree(st);
            return fail(COOLMIC_ERROR_NOMEM, "set_loudness: out of device memory");
        }
        b->d_loud = st;
        b->d_loud_ring = ring;
        b->loud_sub = L;
        b->loud_slots = (unsigned int)R;
        cmhip_loud_coefficients(b->d.rate, b->loud_coef);
    }
    HIP_TRY(hipMemsetAsync(b->d_loud, 0, S * C * sizeof(LoudState), b->stream));
    loud_clear_host(b, 0, S);
    b->loud_on = true;
    return COOLMIC_ERROR_NONE;
}

extern "C" int cmhip_batch_get_loudness(const cmhip_batch_t *b)
{
    if (!b)
        return fail(COOLMIC_ERROR_FAULT, "get_loudness: batch is NULL");
    return b->loud_on ? 1 : 0;
}

static inline unsigned long long loud_completed(const cmhip_batch_t *b, size_t s)
{
    return b->loud_frames[s] / b->loud_sub;
}

// Everything the streams have completed and the host has not taken yet, out of the ring: behind what the stream has
// queued, one copy of the ring, then z_j per sub-block in order.
static int loud_drain(cmhip_batch_t *b)
{
    const size_t S = b->d.streams, C = b->d.channels, R = b->loud_slots;
    bool any = false;
    for (size_t s = 0; s < S && !any; s++)
        any = loud_completed(b, s) != b->loud_drained[s];
    if (!any)
        return COOLMIC_ERROR_NONE;
    HIP_TRY(hipMemcpyAsync(b->loud_host.data(), b->d_loud_ring, S * R * C * sizeof(double), hipMemcpyDeviceToHost,
                           b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    const double L = (double)b->loud_sub;
    for (size_t s = 0; s < S; s++) {
        const unsigned long long done = loud_completed(b, s);
        if (done == b->loud_drained[s])
            continue;
        const double *w = &b->loud_w[s * C];
        // (push_back's own geometric growth: a drain per result call must not copy the stream's whole history)
        try {
            for (unsigned long long j = b->loud_drained[s]; j < done; j++) {
                const double *e = &b->loud_host[(s * R + (size_t)(j % R)) * C];
                double sum = 0.0;
                for (size_t c = 0; c < C; c++)
                    sum += w[c] * e[c];
                b->loud_z[s].push_back(sum / L);
                memcpy(&b->loud_recent[(s * LOUD_RECENT + (size_t)(j % LOUD_RECENT)) * C], e, C * sizeof(double));
                b->loud_drained[s] = j + 1;
            }
        } catch (const std::bad_alloc &) {       // (what was taken so far stays taken; the ring still holds the rest)
            return fail(COOLMIC_ERROR_NOMEM, "loudness: out of host memory for stream %zu's sub-blocks", s);
        }
        b->loud_drained[s] = done;
    }
    return COOLMIC_ERROR_NONE;
}

int cmhip_engine_loud_run(cmhip_batch_t *b, const int16_t *in, size_t frames, const uint32_t *frames_per_stream)
{
    const size_t S = b->d.streams;
    // would this run push a stream's undrained sub-blocks past the ring?  then drain first
    bool full = false;
    for (size_t s = 0; s < S && !full; s++) {
        const unsigned long long n = frames_per_stream ? frames_per_stream[s] : frames;
        full = (b->loud_frames[s] + n) / b->loud_sub - b->loud_drained[s] > b->loud_slots;
    }
    if (full) {
        const int rc = loud_drain(b);
        if (rc != COOLMIC_ERROR_NONE)
            return rc;
    }
    LoudArgs a;
    memset(&a, 0, sizeof(a));
    a.in = in;
    a.param = b->d_param;
    a.nframes = frames_per_stream ? b->d_nframes : nullptr;
    a.state = b->d_loud;
    a.ring = b->d_loud_ring;
    memcpy(a.coef, b->loud_coef, sizeof(a.coef));
    a.frames = (uint32_t)frames;
    a.streams = b->d.streams;
    a.channels = b->d.channels;
    a.sub = b->loud_sub;
    a.ring_slots = b->loud_slots;
    a.stride = b->stride;
    const hipError_t e = launch_loud(a, b->stream);
    if (e != hipSuccess)
        return fail(COOLMIC_ERROR_GENERIC, "run: the loudness pass: %s", hipGetErrorString(e));
    g_loud_runs.fetch_add(1, std::memory_order_relaxed);
    for (size_t s = 0; s < S; s++)
        b->loud_frames[s] += frames_per_stream ? frames_per_stream[s] : frames;
    return COOLMIC_ERROR_NONE;
}

// one stream's result from its drained z
static void loud_finish(const cmhip_batch_t *b, size_t s, coolmic_loudness_result_t *out)
{
    const std::vector<double> &zs = b->loud_z[s];
    const double *z = zs.data();
    const size_t n = zs.size();
    memset(out, 0, sizeof(*out));
    out->rate = b->d.rate;
    out->channels = b->d.channels;
    out->frames = (size_t)b->loud_frames[s];
    out->blocks = n;
    out->momentary = n >= 4 ? cmhip_loud_lufs(loud_block(z, n - 1)) : -INFINITY;
    out->short_term = -INFINITY;
    if (n >= LOUD_RECENT) {
        double sum = 0.0;
        for (size_t i = n - LOUD_RECENT; i < n; i++)
            sum += z[i];
        out->short_term = cmhip_loud_lufs(sum / 30.0);
    }
    (void)cmhip_loud_integrate(z, n, &out->integrated, &out->relative_threshold, &out->gated_blocks);
}

extern "C" int cmhip_batch_loud_result(cmhip_batch_t *b, unsigned int stream, coolmic_loudness_result_t *out)
{
    if (!b || !out)
        return fail(COOLMIC_ERROR_FAULT, "loud_result: NULL argument");
    if (!b->loud_on || stream >= b->d.streams)
        return fail(COOLMIC_ERROR_INVAL, "loud_result: stream out of range or batch without loudness");
    if (use(b))
        return COOLMIC_ERROR_GENERIC;
    const int rc = loud_drain(b);
    if (rc != COOLMIC_ERROR_NONE)
        return rc;
    loud_finish(b, stream, out);
    return COOLMIC_ERROR_NONE;
}

extern "C" int cmhip_batch_loud_results(cmhip_batch_t *b, coolmic_loudness_result_t *out, int *rc)
{
    if (!b || !out)
        return fail(COOLMIC_ERROR_FAULT, "loud_results: NULL argument");
    if (!b->loud_on)
        return fail(COOLMIC_ERROR_INVAL, "loud_results: batch without loudness");
    if (use(b))
        return COOLMIC_ERROR_GENERIC;
    const int r = loud_drain(b);
    if (r != COOLMIC_ERROR_NONE)
        return r;
    for (size_t s = 0; s < b->d.streams; s++) {
        loud_finish(b, s, &out[s]);
        if (rc)
            rc[s] = COOLMIC_ERROR_NONE;
    }
    return COOLMIC_ERROR_NONE;
}

extern "C" int cmhip_batch_loud_raw(cmhip_batch_t *b, unsigned int stream, double *sums, size_t cap, size_t *returned,
                                    unsigned long long *completed)
{
    if (!b || (!sums && cap))
        return fail(COOLMIC_ERROR_FAULT, "loud_raw: NULL argument");
    if (!b->loud_on || stream >= b->d.streams)
        return fail(COOLMIC_ERROR_INVAL, "loud_raw: stream out of range or batch without loudness");
    if (use(b))
        return COOLMIC_ERROR_GENERIC;
    const int rc = loud_drain(b);
    if (rc != COOLMIC_ERROR_NONE)
        return rc;
    const size_t C = b->d.channels;
    const unsigned long long done = b->loud_drained[stream];
    size_t n = cap < LOUD_RECENT ? cap : LOUD_RECENT;
    if (done < n)
        n = (size_t)done;
    for (size_t i = 0; i < n; i++) {
        const unsigned long long j = done - n + i;
        memcpy(sums + i * C, &b->loud_recent[((size_t)stream * LOUD_RECENT + (size_t)(j % LOUD_RECENT)) * C],
               C * sizeof(double));
    }
    if (returned)
        *returned = n;
    if (completed)
        *completed = done;
    return COOLMIC_ERROR_NONE;
}

extern "C" int cmhip_batch_loud_set_weights(cmhip_batch_t *b, long stream, const double *w)
{
    if (!b || !w)
        return fail(COOLMIC_ERROR_FAULT, "loud_set_weights: NULL argument");
    const StreamRange sr = stream_range(stream, b->d.streams);
    if (!b->loud_on || !sr.ok)
        return fail(COOLMIC_ERROR_INVAL, "loud_set_weights: stream %ld out of range or batch without loudness", stream);
    const size_t C = b->d.channels;
    for (size_t c = 0; c < C; c++)
        if (!(w[c] >= 0.0) || !isfinite(w[c]))
            return fail(COOLMIC_ERROR_INVAL, "loud_set_weights: weight %zu is negative or not finite", c);
    const size_t lo = sr.lo, n = sr.n;
    for (size_t s = lo; s < lo + n; s++)
        if (loud_completed(b, s))
            return fail(COOLMIC_ERROR_BUSY, "loud_set_weights: stream %zu holds completed sub-blocks (reset first)", s);
    for (size_t s = lo; s < lo + n; s++)
        memcpy(&b->loud_w[s * C], w, C * sizeof(double));
    return COOLMIC_ERROR_NONE;
}

extern "C" int cmhip_batch_loud_reset(cmhip_batch_t *b, long stream)
{
    if (!b)
        return fail(COOLMIC_ERROR_FAULT, "loud_reset: batch is NULL");
    const StreamRange sr = stream_range(stream, b->d.streams);
    if (!b->loud_on || !sr.ok)
        return fail(COOLMIC_ERROR_INVAL, "loud_reset: stream %ld out of range or batch without loudness", stream);
    if (use(b))
        return COOLMIC_ERROR_GENERIC;
    const size_t C = b->d.channels, lo = sr.lo, n = sr.n;
    HIP_TRY(hipMemsetAsync(b->d_loud + lo * C, 0, n * C * sizeof(LoudState), b->stream));
    loud_clear_host(b, lo, n);
    return COOLMIC_ERROR_NONE;
}
