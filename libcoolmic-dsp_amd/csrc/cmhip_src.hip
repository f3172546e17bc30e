// cmhip_src.hip -- sample-rate conversion on the host side (include/coolmic_hip.h, "sample-rate conversion"): the
// resampler object beside the batch, its validation, the launch of k_src.hip's kernel, the design of the table and
// the two host helpers.
//
// Device state of a resampler: the table in the kernel's form (SrcArgs::table), the streams' history, int16
// [2][S][C][T-1], and their positions r = (frames so far) mod M, uint32 [2][S]; two slots each, selected by a parity
// the host flips per run (HistoryPair, csrc/cmhip_stage.h; the positions follow its parity).  The host keeps a mirror of every r: it knows each
// run's counts, so a run's output counts are known before the call returns, without a device wait.
#include "cmhip_engine.h"
#include "design_window.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <numeric>

constexpr unsigned SRC_MAX_LM = 640, SRC_MAX_T = 192;
constexpr uint64_t SRC_MAX_SAMPLES = 1ull << 31;     // per slot and run: the kernels index a slot in 32 bits

struct cmhip_src : StageBase {
    cmhip_src_desc_t d;
    unsigned L, M, T;
    size_t max_out;                    // floor(max_in_frames * L / M) + 1
    int16_t *d_table;
    HistoryPair hist;                  // [2][S][C * (T-1)]
    uint32_t *d_rpos;                  // [2][S], the slots of hist
    std::vector<uint32_t> r;           // the mirror of the device's current r per stream
};

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

// (the body of cmhip_src_design: its vectors may throw)
static int src_design(unsigned rate_in, unsigned rate_out, unsigned *L, unsigned *M, unsigned *T, int16_t *h, size_t cap)
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
        const double i0b = design_i0(DESIGN_BETA);
        std::vector<double> proto(N);
        for (size_t i = 0; i < N; i++) {
            const double x = (double)i - ((double)N - 1.0) / 2.0;
            proto[i] = design_tap(x, (double)N / 2.0, fc, i0b) * (double)l;      // (csrc/design_window.h)
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

extern "C" int cmhip_src_design(unsigned rate_in, unsigned rate_out, unsigned *L, unsigned *M, unsigned *T, int16_t *h,
                                size_t cap)
{
    return stage_guard("src_design", [&] { return src_design(rate_in, rate_out, L, M, T, h, cap); });
}

static int src_init(cmhip_src_t *r, const int16_t *h)
{
    const cmhip_src_desc_t &d = r->d;
    const size_t S = d.streams;
    // the table as the kernel reads it (SrcArgs::table)
    const unsigned T8 = (r->T + 7u) & ~7u, krow = T8 + 8u;
    std::vector<int16_t> tab((size_t)r->L * krow, 0);
    for (unsigned p = 0; p < r->L; p++)
        for (unsigned k = 0; k < r->T; k += 2) {
            tab[(size_t)p * krow + k] = h[(size_t)p * r->T + k + 1];
            tab[(size_t)p * krow + k + 1] = h[(size_t)p * r->T + k];
        }
    r->r.assign(S, 0);
    if (r->open("src_new", d.device, d.hip_stream, S) || r->alloc("src_new", &r->d_table, tab.size()) ||
        r->array("src_new", &r->d_rpos, 2 * S) || r->hist.init(*r, "src_new", S, (size_t)d.channels * (r->T - 1)))
        return COOLMIC_ERROR_GENERIC;
    HIP_TRY(hipMemcpy(r->d_table, tab.data(), tab.size() * sizeof(int16_t), hipMemcpyHostToDevice));
    return COOLMIC_ERROR_NONE;
}

extern "C" void cmhip_src_free(cmhip_src_t *r) { stage_free(r); }

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
    return stage_new<cmhip_src>("src_new", [&](cmhip_src_t *r) {
        r->d = *d;
        r->L = L;
        r->M = M;
        r->T = T;
        r->max_out = (size_t)max_out;
        return src_init(r, h);
    });
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
    cmhip_src_t *r = nullptr;
    (void)stage_guard("src_new", [&] {
        std::vector<int16_t> h((size_t)L * T);
        if (!src_design(d->rate_in, d->rate_out, nullptr, nullptr, nullptr, h.data(), h.size()))
            r = cmhip_src_new_table(d, L, M, T, h.data());
        return 0;
    });
    return r;
}

extern "C" int cmhip_src_geometry(const cmhip_src_t *r, unsigned *L, unsigned *M, unsigned *T)
{
    if (!r)
        return fail(COOLMIC_ERROR_FAULT, "src_geometry: NULL argument");
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
        const uint32_t k = cmhip_src_out_frames(r->L, r->M, r->r[s], stage_count(frames_per_stream, s, frames));
        if (k > most)
            most = k;
    }
    const StageRun run = {in, out, in_stride, out_stride, frames, r->d.max_in_frames, frames_per_stream, S, S, C, most, C,
                          STAGE_NOT_IN_PLACE};
    int rc;
    const bool go = stage_run_begin(r, "src_run", run, &rc);
    if (rc)
        return rc;
    // nothing was touched so far; from here on the run happens (one of no frames in the mirror alone)
    if (go) {
        SrcArgs a;
        memset(&a, 0, sizeof(a));
        a.in = (const int16_t *)in;
        a.out = (int16_t *)out;
        HIP_TRY(r->send_counts(frames_per_stream, S, &a.nframes));
        a.table = r->d_table;
        a.hist = r->hist.d;
        a.rpos = r->d_rpos;
        a.in_stride = in_stride;
        a.out_stride = out_stride;
        a.frames = (uint32_t)frames;
        a.streams = S;
        a.channels = C;
        a.parity = r->hist.parity();
        a.L = r->L;
        a.M = r->M;
        a.T = r->T;
        // (a run that gives no stream an output still moves history and r: one workgroup per stream)
        rc = stage_launched("src_run", launch_src(a, most ? most : 1u, r->stream));
        if (rc)
            return rc;
        r->hist.flip();                      // the kernel wrote the other slots
    }
    for (unsigned s = 0; s < S; s++) {
        const uint32_t f = stage_count(frames_per_stream, s, frames);
        if (out_frames)
            out_frames[s] = cmhip_src_out_frames(r->L, r->M, r->r[s], f);
        r->r[s] = (uint32_t)(((uint64_t)r->r[s] + f) % r->M);
    }
    return COOLMIC_ERROR_NONE;
}

extern "C" int cmhip_src_reset(cmhip_src_t *r, long stream)
{
    StreamRange sr;
    const int rc = stage_streams(r, "src_reset", stream, &sr);
    if (rc)
        return rc;
    HIP_TRY(hipSetDevice(r->d.device));
    HIP_TRY(r->hist.reset(sr.lo, sr.n, r->stream));
    HIP_TRY(hipMemsetAsync(r->d_rpos + r->hist.slots.at(sr.lo, 1), 0, sr.n * sizeof(uint32_t), r->stream));
    for (size_t s = sr.lo; s < (size_t)sr.lo + sr.n; s++)
        r->r[s] = 0;
    return COOLMIC_ERROR_NONE;
}
