// cmhip_split.hip -- the band split on the host side (include/coolmic_hip.h, "band split"): the object beside the batch,
// its validation, the launch of k_split.hip's kernels, the design of the filters and the table check.
//
// Device state of a band split: the filters in the kernel's form (csrc/split_plan.h), the streams' history, int16
// [2][S][C][T-1], two slots selected by a parity the host flips per run (HistoryPair, csrc/cmhip_stage.h), and the clip
// counters, uint32 [S][B].  The host keeps the filters as the caller gave them; cmhip_split_get_table answers from them.
#include "cmhip_engine.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>

constexpr uint64_t SPLIT_MAX_SAMPLES = 1ull << 31;   // per slot and run: the kernels index a slot in 32 bits

struct cmhip_split : StageBase {
    cmhip_split_desc_t d;
    std::vector<int16_t> g;            // [B-1][T] as the caller gave them
    std::vector<uint8_t> q;            // [B-1]
    uint32_t *d_table;
    HistoryPair hist;                  // [2][S][C * (T-1)]
    uint32_t *d_clips;                 // [S][B]
};

static int split_geometry(const char *who, unsigned bands, unsigned taps)
{
    if (!split_geometry_ok(bands, taps))
        return fail(COOLMIC_ERROR_INVAL, "%s: %u bands of %u taps: bands must lie in 2..8, taps must be odd and lie in 3..1023",
                    who, bands, taps);
    return COOLMIC_ERROR_NONE;
}

extern "C" int cmhip_split_check(unsigned bands, unsigned taps, const int16_t *g, const uint8_t *q)
{
    const int rc = split_geometry("split_check", bands, taps);
    if (rc)
        return rc;
    if (!g || !q)
        return fail(COOLMIC_ERROR_FAULT, "split_check: NULL argument");
    for (unsigned b = 0; b + 1 < bands; b++)
        if (q[b] < SPLIT_Q_MIN || q[b] > SPLIT_Q_MAX)
            return fail(COOLMIC_ERROR_INVAL, "split_check: q[%u] = %u: must lie in 14..20", b, (unsigned)q[b]);
    return COOLMIC_ERROR_NONE;
}

// I0 from its power series, summed until a term no longer changes the sum (cmhip_src_design's)
static double split_i0(double x)
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

// (the body of cmhip_split_design: its vectors may throw)
static int split_design(unsigned rate, unsigned bands, const double *crossover_hz, unsigned taps, int16_t *g, uint8_t *q,
                        size_t cap)
{
    const int rc = split_geometry("split_design", bands, taps);
    if (rc)
        return rc;
    if (!crossover_hz || (g && !q))
        return fail(COOLMIC_ERROR_FAULT, "split_design: NULL argument");
    const unsigned nf = bands - 1, T = taps, D = (T - 1) / 2;
    for (unsigned j = 0; j < nf; j++) {
        const double f = crossover_hz[j], below = j ? crossover_hz[j - 1] : 0.0;
        if (rate == 0 || !(f > below) || !(f < (double)rate / 2.0))
            return fail(COOLMIC_ERROR_INVAL, "split_design: crossover %u must lie above the one before and inside (0, rate/2)", j);
    }
    if (!g)
        return COOLMIC_ERROR_NONE;
    if (cap < (size_t)nf * T)
        return fail(COOLMIC_ERROR_INVAL, "split_design: room for %zu entries, the filters have %zu", cap, (size_t)nf * T);
    // the cumulative low-passes, each divided by its own sum
    const double i0b = split_i0(7.5);
    std::vector<double> l((size_t)nf * T), h((size_t)nf * T);
    for (unsigned j = 0; j < nf; j++) {
        const double fc = crossover_hz[j] / (double)rate;
        double sum = 0.0;
        for (unsigned i = 0; i < T; i++) {
            const double x = (double)i - (double)D;
            const double u = x / ((double)D + 1.0);
            const double arg = 1.0 - u * u;
            const double w = split_i0(7.5 * sqrt(arg > 0.0 ? arg : 0.0)) / i0b;
            const double ts = 2.0 * fc * x;
            const double sinc = ts == 0.0 ? 1.0 : sin(M_PI * ts) / (M_PI * ts);
            l[(size_t)j * T + i] = 2.0 * fc * sinc * w;
            sum += l[(size_t)j * T + i];
        }
        for (unsigned i = 0; i < T; i++)
            l[(size_t)j * T + i] /= sum;
    }
    for (unsigned j = 0; j < nf; j++)
        for (unsigned i = 0; i < T; i++)
            h[(size_t)j * T + i] = l[(size_t)j * T + i] - (j ? l[(size_t)(j - 1) * T + i] : 0.0);
    // per filter the largest q whose finished taps stay within +-32767
    std::vector<int16_t> tab((size_t)nf * T);
    std::vector<uint8_t> qs(nf);
    std::vector<long> t(T);
    for (unsigned j = 0; j < nf; j++) {
        unsigned qq = SPLIT_Q_MAX;
        for (;; qq--) {
            long isum = 0;
            for (unsigned i = 0; i < T; i++) {
                t[i] = (long)rint(h[(size_t)j * T + i] * (double)(1u << qq));
                isum += t[i];
            }
            t[D] += (j == 0 ? (1l << qq) : 0l) - isum;
            bool fits = true;
            for (unsigned i = 0; i < T; i++)
                fits = fits && t[i] >= -32767 && t[i] <= 32767;
            if (fits)
                break;
            if (qq == SPLIT_Q_MIN)
                return fail(COOLMIC_ERROR_GENERIC, "split_design: a coefficient left int16");
        }
        qs[j] = (uint8_t)qq;
        for (unsigned i = 0; i < T; i++)
            tab[(size_t)j * T + i] = (int16_t)t[i];
    }
    memcpy(g, tab.data(), tab.size() * sizeof(int16_t));
    memcpy(q, qs.data(), nf);
    return COOLMIC_ERROR_NONE;
}

extern "C" int cmhip_split_design(unsigned rate, unsigned bands, const double *crossover_hz, unsigned taps, int16_t *g,
                                  uint8_t *q, size_t cap)
{
    return stage_guard("split_design", [&] { return split_design(rate, bands, crossover_hz, taps, g, q, cap); });
}

static int split_init(cmhip_split_t *m)
{
    const cmhip_split_desc_t &d = m->d;
    const size_t S = d.streams;
    std::vector<uint32_t> tab((split_table_words(d.bands, d.taps) + 3u) & ~3u, 0);
    split_compile(d.bands, d.taps, m->g.data(), m->q.data(), tab.data());
    if (m->open("split_new", d.device, d.hip_stream, S) || m->alloc("split_new", &m->d_table, tab.size()) ||
        m->array("split_new", &m->d_clips, S * d.bands) ||
        m->hist.init(*m, "split_new", S, (size_t)d.channels * (d.taps - 1)))
        return COOLMIC_ERROR_GENERIC;
    HIP_TRY(hipMemcpy(m->d_table, tab.data(), tab.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    return COOLMIC_ERROR_NONE;
}

extern "C" void cmhip_split_free(cmhip_split_t *m) { stage_free(m); }

extern "C" cmhip_split_t *cmhip_split_new_table(const cmhip_split_desc_t *d, const int16_t *g, const uint8_t *q)
{
    if (!d || !g || !q) {
        fail(COOLMIC_ERROR_FAULT, "split_new: NULL argument");
        return nullptr;
    }
    if (d->streams == 0 || d->channels == 0 || d->channels > MAX_CH || d->max_frames == 0) {
        fail(COOLMIC_ERROR_INVAL, "split_new: streams, channels (1..16) and max_frames must be positive");
        return nullptr;
    }
    if (cmhip_split_check(d->bands, d->taps, g, q))
        return nullptr;
    if ((uint64_t)d->max_frames * d->channels > SPLIT_MAX_SAMPLES) {
        fail(COOLMIC_ERROR_INVAL, "split_new: max_frames %zu: a slot of a run would pass 2^31 samples", d->max_frames);
        return nullptr;
    }
    if ((uint64_t)d->streams * d->bands >= (1ull << 31)) {
        fail(COOLMIC_ERROR_INVAL, "split_new: %u streams of %u bands: the output would pass 2^31 slots", d->streams, d->bands);
        return nullptr;
    }
    return stage_new<cmhip_split>("split_new", [&](cmhip_split_t *m) {
        m->d = *d;
        const size_t nf = d->bands - 1;
        m->g.assign(g, g + nf * d->taps);
        m->q.assign(q, q + nf);
        return split_init(m);
    });
}

extern "C" cmhip_split_t *cmhip_split_new(const cmhip_split_desc_t *d, unsigned rate, const double *crossover_hz)
{
    if (!d || !crossover_hz) {
        fail(COOLMIC_ERROR_FAULT, "split_new: NULL argument");
        return nullptr;
    }
    if (split_geometry("split_new", d->bands, d->taps))
        return nullptr;
    cmhip_split_t *m = nullptr;
    (void)stage_guard("split_new", [&] {
        std::vector<int16_t> g((size_t)(d->bands - 1) * d->taps);
        std::vector<uint8_t> q(d->bands - 1);
        if (!split_design(rate, d->bands, crossover_hz, d->taps, g.data(), q.data(), g.size()))
            m = cmhip_split_new_table(d, g.data(), q.data());
        return 0;
    });
    return m;
}

extern "C" unsigned cmhip_split_delay(const cmhip_split_t *m) { return m ? (m->d.taps - 1) / 2 : 0; }

extern "C" int cmhip_split_get_table(const cmhip_split_t *m, int16_t *g, uint8_t *q)
{
    if (!m || !g || !q)
        return fail(COOLMIC_ERROR_FAULT, "split_get_table: NULL argument");
    memcpy(g, m->g.data(), m->g.size() * sizeof(int16_t));
    memcpy(q, m->q.data(), m->q.size());
    return COOLMIC_ERROR_NONE;
}

extern "C" void *cmhip_split_hip_stream(cmhip_split_t *m) { return m ? (void *)m->stream : nullptr; }

extern "C" int cmhip_split_sync(cmhip_split_t *m) { return stage_sync(m, "split_sync"); }

extern "C" int cmhip_split_run(cmhip_split_t *m, const void *in, size_t in_stride, size_t frames,
                               const uint32_t *frames_per_stream, void *out, size_t out_stride)
{
    if (!m)
        return fail(COOLMIC_ERROR_FAULT, "split_run: NULL argument");
    const unsigned S = m->d.streams, C = m->d.channels, B = m->d.bands;
    const StageRun r = {in, out, in_stride, out_stride, frames, m->d.max_frames, frames_per_stream, S, (size_t)B * S, C,
                        frames, C, STAGE_APART};
    int rc;
    if (!stage_run_begin(m, "split_run", r, &rc))
        return rc;
    if (plan_split(S, C, B, m->d.taps, (uint32_t)frames).err)
        return fail(COOLMIC_ERROR_INVAL, "split_run: %u streams of %zu frames: the grid would reach 2^31 workgroups", S, frames);
    // nothing was touched so far; from here on the run happens
    SplitArgs a;
    memset(&a, 0, sizeof(a));
    a.in = (const int16_t *)in;
    a.out = (int16_t *)out;
    HIP_TRY(m->send_counts(frames_per_stream, S, &a.nframes));
    a.table = m->d_table;
    a.hist = m->hist.d;
    a.clips = m->d_clips;
    a.in_stride = in_stride;
    a.out_stride = out_stride;
    a.frames = (uint32_t)frames;
    a.streams = S;
    a.channels = C;
    a.bands = B;
    a.taps = m->d.taps;
    a.parity = m->hist.parity();
    rc = stage_launched("split_run", launch_split(a, m->stream));
    if (!rc)
        m->hist.flip();                      // the kernel wrote the other slot
    return rc;
}

extern "C" int cmhip_split_reset(cmhip_split_t *m, long stream)
{
    StreamRange sr;
    const int rc = stage_streams(m, "split_reset", stream, &sr);
    if (rc)
        return rc;
    HIP_TRY(hipSetDevice(m->d.device));
    const size_t B = m->d.bands;
    HIP_TRY(m->hist.reset(sr.lo, sr.n, m->stream));
    HIP_TRY(hipMemsetAsync(m->d_clips + sr.lo * B, 0, sr.n * B * sizeof(uint32_t), m->stream));
    return COOLMIC_ERROR_NONE;
}

extern "C" int cmhip_split_clips(cmhip_split_t *m, uint32_t *clips, int clear)
{
    if (!m || !clips)
        return fail(COOLMIC_ERROR_FAULT, "split_clips: NULL argument");
    return stage_read(m, clips, m->d_clips, (size_t)m->d.streams * m->d.bands * sizeof(uint32_t), clear != 0);
}
