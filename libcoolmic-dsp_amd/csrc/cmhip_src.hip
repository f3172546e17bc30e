// cmhip_src.hip -- sample-rate conversion on the host side (include/coolmic_hip.h, "sample-rate conversion"): the
// resampler object beside the batch, its validation, the launch of k_src.hip's kernel, the design of the table and
// the two host helpers.
//
// Device state of a resampler: the table in the kernel's form (SrcArgs::table), the streams' history, int16
// [2][S][C][T-1], and their positions r = (frames so far) mod M, uint32 [2][S]; two slots each, selected by a parity
// the host flips per run (the mechanism of the true-peak history).  The host keeps a mirror of every r: it knows each
// run's counts, so a run's output counts are known before the call returns, without a device wait.
#include "cmhip_engine.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <new>
#include <numeric>

constexpr unsigned SRC_MAX_LM = 640, SRC_MAX_T = 192;
constexpr uint64_t SRC_MAX_SAMPLES = 1ull << 31;     // per slot and run: the kernels index a slot in 32 bits

struct cmhip_src : StageBase {
    cmhip_src_desc_t d;
    unsigned L, M, T;
    size_t max_out;                    // floor(max_in_frames * L / M) + 1
    int16_t *d_table;
    int16_t *d_hist;
    uint32_t *d_rpos;
    unsigned parity;
    std::vector<uint32_t> r;           // the mirror of the device's current r per stream
};

static size_t src_hist_words(const cmhip_src_t *r) { return (size_t)r->d.streams * r->d.channels * (r->T - 1); }

extern "C" uint32_t cmhip_src_out_frames(unsigned L, unsigned M, uint32_t r, uint32_t frames)
{
    if (L == 0 || M == 0)
        return 0;
    const uint64_t before = ((uint64_t)r * L + M - 1) / M;
    const uint64_t after = (((uint64_t)r + frames) * L + M - 1) / M;
    return (uint32_t)(after - before);
}

// L, M in 1..640 and different, T even in 2..192, every phase with sum |h| <= 65535: then |acc + 8192| < 2^31
static int src_table_check(unsigned L, unsigned M, unsigned T, const int16_t *h)
{
    if (L < 1 || L > SRC_MAX_LM || M < 1 || M > SRC_MAX_LM || L == M)
        return fail(COOLMIC_ERROR_INVAL, "src: L = %u, M = %u: both must lie in 1..640 and differ", L, M);
    if (T < 2 || T > SRC_MAX_T || (T & 1))
        return fail(COOLMIC_ERROR_INVAL, "src: T = %u: must be even and lie in 2..192", T);
    for (unsigned p = 0; p < L; p++) {
        unsigned long sum = 0;
        for (unsigned k = 0; k < T; k++)
            sum += (unsigned long)abs((int)h[(size_t)p * T + k]);
        if (sum > 65535)
            return fail(COOLMIC_ERROR_INVAL, "src: phase %u has sum |h| = %lu above 65535", p, sum);
    }
    return COOLMIC_ERROR_NONE;
}

static int src_geometry(unsigned rate_in, unsigned rate_out, unsigned *L, unsigned *M, unsigned *T)
{
    if (rate_in == 0 || rate_out == 0 || rate_in == rate_out)
        return fail(COOLMIC_ERROR_INVAL, "src: rates %u -> %u: both must be positive and differ", rate_in, rate_out);
    const unsigned g = std::gcd(rate_in, rate_out);
    *L = rate_out / g;
    *M = rate_in / g;
    if (*L > SRC_MAX_LM || *M > SRC_MAX_LM)
        return fail(COOLMIC_ERROR_INVAL, "src: rates %u -> %u reduce to %u / %u, above 640", rate_in, rate_out, *L, *M);
    *T = *L > *M ? 32u : 32u * ((*M + *L - 1) / *L);
    return COOLMIC_ERROR_NONE;
}

// I0 from its power series, summed until a term no longer changes the sum
static double src_i0(double x)
{
    double sum = 1.0, t = 1.0;
    for (unsigned k = 1;; k++) {
        t = t * (x / 2.0) / (double)k;
        const double next = sum + t * t;
        if (next == sum)
            return sum;
        sum = next;
    }
}

extern "C" int cmhip_src_design(unsigned rate_in, unsigned rate_out, unsigned *L, unsigned *M, unsigned *T, int16_t *h,
                                size_t cap)
{
    unsigned l, m, t;
    const int rc = src_geometry(rate_in, rate_out, &l, &m, &t);
    if (rc)
        return rc;
    const size_t N = (size_t)l * t;
    if (h) {
        if (cap < N)
            return fail(COOLMIC_ERROR_INVAL, "src_design: room for %zu entries, the table has %zu", cap, N);
        const double fc = 0.92 * 0.5 / (double)(l > m ? l : m);
        const double i0b = src_i0(7.5);
        std::vector<double> proto(N);
        for (size_t i = 0; i < N; i++) {
            const double x = (double)i - ((double)N - 1.0) / 2.0;
            const double u = x / ((double)N / 2.0);
            const double arg = 1.0 - u * u;
            const double w = src_i0(7.5 * sqrt(arg > 0.0 ? arg : 0.0)) / i0b;
            const double ts = 2.0 * fc * x;
            const double sinc = ts == 0.0 ? 1.0 : sin(M_PI * ts) / (M_PI * ts);
            proto[i] = 2.0 * fc * sinc * w * (double)l;
        }
        std::vector<int16_t> tab(N);
        for (unsigned p = 0; p < l; p++) {
            double sum = 0.0;
            for (unsigned k = 0; k < t; k++)
                sum += proto[(size_t)k * l + p];
            long isum = 0, q[SRC_MAX_T];
            unsigned big = 0;
            for (unsigned k = 0; k < t; k++) {
                q[k] = (long)rint(proto[(size_t)k * l + p] / sum * 16384.0);
                isum += q[k];
                if (labs(q[k]) > labs(q[big]))
                    big = k;                                 // the first tap of largest magnitude
            }
            q[big] += 16384 - isum;
            for (unsigned k = 0; k < t; k++) {
                if (q[k] < -32768 || q[k] > 32767)
                    return fail(COOLMIC_ERROR_GENERIC, "src_design: a coefficient left int16");
                tab[(size_t)p * t + k] = (int16_t)q[k];
            }
        }
        if (src_table_check(l, m, t, tab.data()))
            return COOLMIC_ERROR_GENERIC;
        memcpy(h, tab.data(), N * sizeof(int16_t));
    }
    if (L)
        *L = l;
    if (M)
        *M = m;
    if (T)
        *T = t;
    return COOLMIC_ERROR_NONE;
}

static int src_init(cmhip_src_t *r, const int16_t *h)
{
    const cmhip_src_desc_t &d = r->d;
    if (r->open(d.device, d.hip_stream, d.streams))
        return COOLMIC_ERROR_GENERIC;
    // the table as the kernel reads it (SrcArgs::table)
    const unsigned T8 = (r->T + 7u) & ~7u, krow = T8 + 8u;
    std::vector<int16_t> tab((size_t)r->L * krow, 0);
    for (unsigned p = 0; p < r->L; p++)
        for (unsigned k = 0; k < r->T; k += 2) {
            tab[(size_t)p * krow + k] = h[(size_t)p * r->T + k + 1];
            tab[(size_t)p * krow + k + 1] = h[(size_t)p * r->T + k];
        }
    const size_t S = d.streams;
    HIP_TRY(hipMalloc((void **)&r->d_table, tab.size() * sizeof(int16_t)));
    HIP_TRY(hipMalloc((void **)&r->d_hist, 2 * src_hist_words(r) * sizeof(int16_t)));
    HIP_TRY(hipMalloc((void **)&r->d_rpos, 2 * S * sizeof(uint32_t)));
    HIP_TRY(hipMemcpy(r->d_table, tab.data(), tab.size() * sizeof(int16_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemsetAsync(r->d_hist, 0, 2 * src_hist_words(r) * sizeof(int16_t), r->stream));
    HIP_TRY(hipMemsetAsync(r->d_rpos, 0, 2 * S * sizeof(uint32_t), r->stream));
    r->r.assign(S, 0);
    return COOLMIC_ERROR_NONE;
}

extern "C" void cmhip_src_free(cmhip_src_t *r)
{
    if (!r)
        return;
    r->close();
    (void)hipFree(r->d_table);
    (void)hipFree(r->d_hist);
    (void)hipFree(r->d_rpos);
    delete r;
}

extern "C" cmhip_src_t *cmhip_src_new_table(const cmhip_src_desc_t *d, unsigned L, unsigned M, unsigned T,
                                            const int16_t *h)
{
    if (!d || !h) {
        fail(COOLMIC_ERROR_FAULT, "src_new: NULL argument");
        return nullptr;
    }
    if (d->streams == 0 || d->channels == 0 || d->channels > MAX_CH || d->max_in_frames == 0) {
        fail(COOLMIC_ERROR_INVAL, "src_new: streams, channels (1..16) and max_in_frames must be positive");
        return nullptr;
    }
    if (src_table_check(L, M, T, h))
        return nullptr;
    const uint64_t max_out = (uint64_t)d->max_in_frames * L / M + 1;
    if ((uint64_t)d->max_in_frames * d->channels > SRC_MAX_SAMPLES || max_out * d->channels > SRC_MAX_SAMPLES) {
        fail(COOLMIC_ERROR_INVAL, "src_new: max_in_frames %zu: a slot of a run would pass 2^31 samples", d->max_in_frames);
        return nullptr;
    }
    cmhip_src_t *r = new (std::nothrow) cmhip_src();
    if (!r) {
        fail(COOLMIC_ERROR_NOMEM, "src_new: out of memory");
        return nullptr;
    }
    r->d = *d;
    r->L = L;
    r->M = M;
    r->T = T;
    r->max_out = (size_t)max_out;
    if (src_init(r, h)) {
        cmhip_src_free(r);
        return nullptr;
    }
    return r;
}

extern "C" cmhip_src_t *cmhip_src_new(const cmhip_src_desc_t *d)
{
    if (!d) {
        fail(COOLMIC_ERROR_FAULT, "src_new: NULL argument");
        return nullptr;
    }
    unsigned L, M, T;
    if (src_geometry(d->rate_in, d->rate_out, &L, &M, &T))
        return nullptr;
    std::vector<int16_t> h((size_t)L * T);
    if (cmhip_src_design(d->rate_in, d->rate_out, nullptr, nullptr, nullptr, h.data(), h.size()))
        return nullptr;
    return cmhip_src_new_table(d, L, M, T, h.data());
}

extern "C" int cmhip_src_geometry(const cmhip_src_t *r, unsigned *L, unsigned *M, unsigned *T)
{
    if (!r)
        return fail(COOLMIC_ERROR_FAULT, "src_geometry: resampler is NULL");
    if (L)
        *L = r->L;
    if (M)
        *M = r->M;
    if (T)
        *T = r->T;
    return COOLMIC_ERROR_NONE;
}

extern "C" size_t cmhip_src_max_out_frames(const cmhip_src_t *r) { return r ? r->max_out : 0; }
extern "C" void *cmhip_src_hip_stream(cmhip_src_t *r) { return r ? (void *)r->stream : nullptr; }

extern "C" int cmhip_src_sync(cmhip_src_t *r) { return stage_sync(r, "src_sync"); }

extern "C" int cmhip_src_run(cmhip_src_t *r, const void *in, size_t in_stride, size_t frames,
                             const uint32_t *frames_per_stream, void *out, size_t out_stride, uint32_t *out_frames)
{
    if (!r)
        return fail(COOLMIC_ERROR_FAULT, "src_run: NULL argument");
    const unsigned S = r->d.streams, C = r->d.channels;
    // what the run gives its longest stream (pure arithmetic on counts the check below has yet to judge)
    uint32_t most = 0;
    for (unsigned s = 0; s < S; s++) {
        const uint32_t f = frames_per_stream ? frames_per_stream[s] : (uint32_t)frames;
        const uint32_t k = cmhip_src_out_frames(r->L, r->M, r->r[s], f);
        if (k > most)
            most = k;
    }
    const StageRun run = {in, out, in_stride, out_stride, frames, r->d.max_in_frames, frames_per_stream, S, S, C, most, C,
                          STAGE_NOT_IN_PLACE};
    const int refused = stage_run_refusal("src_run", run);
    if (refused)
        return refused;
    // nothing was touched so far; from here on the run happens
    HIP_TRY(hipSetDevice(r->d.device));
    if (frames > 0) {
        if (frames_per_stream)
            HIP_TRY(r->counts.upload(r->d_counts, frames_per_stream, S, r->stream));
        SrcArgs a;
        memset(&a, 0, sizeof(a));
        a.in = (const int16_t *)in;
        a.out = (int16_t *)out;
        a.nframes = frames_per_stream ? r->d_counts : nullptr;
        a.table = r->d_table;
        a.hist = r->d_hist;
        a.rpos = r->d_rpos;
        a.in_stride = in_stride;
        a.out_stride = out_stride;
        a.frames = (uint32_t)frames;
        a.streams = S;
        a.channels = C;
        a.parity = r->parity;
        a.L = r->L;
        a.M = r->M;
        a.T = r->T;
        // (a run that gives no stream an output still moves history and r: one workgroup per stream)
        const hipError_t e = launch_src(a, most ? most : 1u, r->stream);
        if (e != hipSuccess)
            return fail(COOLMIC_ERROR_GENERIC, "src_run: %s", hipGetErrorString(e));
        r->parity ^= 1u;                     // the kernel wrote the other slots
    }
    for (unsigned s = 0; s < S; s++) {
        const uint32_t f = frames_per_stream ? frames_per_stream[s] : (uint32_t)frames;
        if (out_frames)
            out_frames[s] = cmhip_src_out_frames(r->L, r->M, r->r[s], f);
        r->r[s] = (uint32_t)(((uint64_t)r->r[s] + f) % r->M);
    }
    return COOLMIC_ERROR_NONE;
}

extern "C" int cmhip_src_reset(cmhip_src_t *r, long stream)
{
    if (!r)
        return fail(COOLMIC_ERROR_FAULT, "src_reset: resampler is NULL");
    const StreamRange sr = stream_range(stream, r->d.streams);
    if (!sr.ok)
        return fail(COOLMIC_ERROR_INVAL, "src_reset: stream %ld out of range", stream);
    HIP_TRY(hipSetDevice(r->d.device));
    const size_t S = r->d.streams, per = (size_t)r->d.channels * (r->T - 1);
    const size_t lo = sr.lo, n = sr.n;
    for (unsigned slot = 0; slot < 2; slot++) {
        HIP_TRY(hipMemsetAsync(r->d_hist + slot * src_hist_words(r) + lo * per, 0, n * per * sizeof(int16_t), r->stream));
        HIP_TRY(hipMemsetAsync(r->d_rpos + slot * S + lo, 0, n * sizeof(uint32_t), r->stream));
    }
    for (size_t s = lo; s < lo + n; s++)
        r->r[s] = 0;
    return COOLMIC_ERROR_NONE;
}
