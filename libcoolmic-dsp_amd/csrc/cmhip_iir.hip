// cmhip_iir.hip -- the filter stage on the host side (include/coolmic_hip.h, "filter"): the object beside the batch,
// its validation, the host's mirror of every stream's coefficients, the design of sections from the cookbook's
// formulas, the response of a cascade of integers, and the launch of k_iir.hip's kernels.
//
// Device state of a filter: per row and section the histories and the remainder (IirState), per stream the two
// counters, and the coefficient table.  The table lies behind the run's counts in one device array and travels with
// them through the counts ring, but only in a run that follows a set or a ramp: both change the mirror alone and are
// ordered with the runs by the order of the calls.  A reset is a memset of the stream's rows on the object's stream.
//
// Coefficient ramps (csrc/iir_ramp.h): the mirror holds per section both ends, done and R, and advances by every run's
// counts, which the host knows; the device keeps nothing of a ramp.  While any section ramps the table that travels is
// the mirror as it is, IIR_RAMP_WORDS per section, and the kernels are k_iirramp.hip's; a run at whose start nothing
// ramps sends the five words per section, and only if they changed, and launches what it always did.
#include "cmhip_engine.h"

#include <math.h>
#include <string.h>

static_assert(sizeof(cmhip_iir_section_t) == sizeof(IirSec) && sizeof(IirSec) == 20, "cmhip_iir_section_t is IirSec");
static_assert(offsetof(cmhip_iir_section_t, a1) == offsetof(IirSec, a1), "cmhip_iir_section_t is IirSec");
static_assert(CMHIP_IIR_ONE == IIR_ONE, "the coefficient unit");

struct cmhip_iir : StageBase {
    cmhip_iir_desc_t d;
    IirRampMirror ramp;                // [S][N] the mirror: the sections, at rest or between two ends
    bool dirty;                        // the sections in force are not the five-word table the device last got
    IirState *d_state;                 // [S * C][N]
    unsigned long long *d_clips;       // [S]
    unsigned long long *d_overs;       // [S]
};

static IirSec iir_from(const cmhip_iir_section_t *p)
{
    IirSec q;
    memcpy(&q, p, sizeof(q));
    return q;
}

extern "C" int cmhip_iir_check(const cmhip_iir_section_t *c)
{
    if (!c)
        return fail(COOLMIC_ERROR_FAULT, "iir_check: NULL argument");
    if (!iir_section_ok(iir_from(c)))
        return fail(COOLMIC_ERROR_INVAL, "iir_check: every |c| <= 2^28, |a2| < 2^26 and |a1| < 2^26 + a2 are required");
    return COOLMIC_ERROR_NONE;
}

extern "C" int cmhip_iir_design(const cmhip_iir_design_desc_t *d, cmhip_iir_section_t *out)
{
    if (!d || !out)
        return fail(COOLMIC_ERROR_FAULT, "iir_design: NULL argument");
    if (!isfinite(d->rate) || !isfinite(d->f0) || !isfinite(d->q) || !isfinite(d->gain_db))
        return fail(COOLMIC_ERROR_INVAL, "iir_design: a value is not finite");
    if (d->kind < CMHIP_IIR_BYPASS || d->kind > CMHIP_IIR_LOWPASS1)
        return fail(COOLMIC_ERROR_INVAL, "iir_design: unknown kind %d", d->kind);
    if (!(d->rate > 0.0) || !(d->f0 > 0.0) || !(d->f0 < d->rate / 2.0) || !(d->q > 0.0))
        return fail(COOLMIC_ERROR_INVAL, "iir_design: f0 must lie inside (0, rate / 2) and q above 0");
    const double w0 = 2.0 * M_PI * d->f0 / d->rate, cs = cos(w0), sn = sin(w0), alpha = sn / (2.0 * d->q);
    const double A = pow(10.0, d->gain_db / 40.0), sq = 2.0 * sqrt(A) * alpha;
    double b0 = 1.0, b1 = 0.0, b2 = 0.0, a0 = 1.0, a1 = 0.0, a2 = 0.0;
    switch (d->kind) {
    case CMHIP_IIR_BYPASS:
        break;
    case CMHIP_IIR_HIGHPASS:
        b0 = (1.0 + cs) / 2.0; b1 = -(1.0 + cs); b2 = (1.0 + cs) / 2.0;
        a0 = 1.0 + alpha; a1 = -2.0 * cs; a2 = 1.0 - alpha;
        break;
    case CMHIP_IIR_LOWPASS:
        b0 = (1.0 - cs) / 2.0; b1 = 1.0 - cs; b2 = (1.0 - cs) / 2.0;
        a0 = 1.0 + alpha; a1 = -2.0 * cs; a2 = 1.0 - alpha;
        break;
    case CMHIP_IIR_LOWSHELF:
        b0 = A * ((A + 1.0) - (A - 1.0) * cs + sq); b1 = 2.0 * A * ((A - 1.0) - (A + 1.0) * cs);
        b2 = A * ((A + 1.0) - (A - 1.0) * cs - sq);
        a0 = (A + 1.0) + (A - 1.0) * cs + sq; a1 = -2.0 * ((A - 1.0) + (A + 1.0) * cs); a2 = (A + 1.0) + (A - 1.0) * cs - sq;
        break;
    case CMHIP_IIR_HIGHSHELF:
        b0 = A * ((A + 1.0) + (A - 1.0) * cs + sq); b1 = -2.0 * A * ((A - 1.0) + (A + 1.0) * cs);
        b2 = A * ((A + 1.0) + (A - 1.0) * cs - sq);
        a0 = (A + 1.0) - (A - 1.0) * cs + sq; a1 = 2.0 * ((A - 1.0) - (A + 1.0) * cs); a2 = (A + 1.0) - (A - 1.0) * cs - sq;
        break;
    case CMHIP_IIR_PEAK:
        b0 = 1.0 + alpha * A; b1 = -2.0 * cs; b2 = 1.0 - alpha * A;
        a0 = 1.0 + alpha / A; a1 = -2.0 * cs; a2 = 1.0 - alpha / A;
        break;
    case CMHIP_IIR_NOTCH:
        b0 = 1.0; b1 = -2.0 * cs; b2 = 1.0;
        a0 = 1.0 + alpha; a1 = -2.0 * cs; a2 = 1.0 - alpha;
        break;
    case CMHIP_IIR_HIGHPASS1:
    case CMHIP_IIR_LOWPASS1: {
        const double K = tan(w0 / 2.0);
        a0 = 1.0 + K; a1 = K - 1.0;
        if (d->kind == CMHIP_IIR_HIGHPASS1) {
            b0 = 1.0; b1 = -1.0;
        } else {
            b0 = K; b1 = K;
        }
        break;
    }
    }
    const double c[5] = {b0 / a0, b1 / a0, b2 / a0, a1 / a0, a2 / a0};
    int64_t n[5];
    for (int i = 0; i < 5; i++) {
        const double v = rint(c[i] * (double)IIR_ONE);
        if (!isfinite(v) || fabs(v) > (double)IIR_COEF_MAX)
            return fail(COOLMIC_ERROR_INVAL, "iir_design: a coefficient of %g is outside +-4", c[i]);
        n[i] = (int64_t)v;
    }
    // the zero at DC on z = 1 exactly
    if (d->kind == CMHIP_IIR_HIGHPASS)
        n[1] = -(n[0] + n[2]);
    if (d->kind == CMHIP_IIR_HIGHPASS1)
        n[1] = -n[0];
    const IirSec s = {(int32_t)n[0], (int32_t)n[1], (int32_t)n[2], (int32_t)n[3], (int32_t)n[4]};
    if (!iir_section_ok(s))
        return fail(COOLMIC_ERROR_INVAL, "iir_design: the rounded section lies outside the stability triangle");
    memcpy(out, &s, sizeof(s));
    return COOLMIC_ERROR_NONE;
}

extern "C" double cmhip_iir_response_db(const cmhip_iir_section_t *sec, unsigned int n, double rate, double f)
{
    if (!sec || !(rate > 0.0) || !isfinite(f) || !isfinite(rate))
        return NAN;
    const double w = 2.0 * M_PI * f / rate;
    const double c1 = cos(w), s1 = sin(w), c2 = cos(2.0 * w), s2 = sin(2.0 * w), one = (double)IIR_ONE;
    double db = 0.0;
    for (unsigned i = 0; i < n; i++) {
        const double nr = sec[i].b0 + sec[i].b1 * c1 + sec[i].b2 * c2, ni = -(sec[i].b1 * s1 + sec[i].b2 * s2);
        const double dr = one + sec[i].a1 * c1 + sec[i].a2 * c2, di = -(sec[i].a1 * s1 + sec[i].a2 * s2);
        db += 10.0 * log10((nr * nr + ni * ni) / (dr * dr + di * di));
    }
    return db;
}

extern "C" void cmhip_iir_free(cmhip_iir_t *m) { stage_free(m); }

static size_t iir_table_words(const cmhip_iir_desc_t &d, bool ramp)
{
    return (size_t)d.streams * d.sections * (ramp ? IIR_RAMP_WORDS : IIR_SEC_WORDS);
}

// device false (cmhip_test_iir_new_dry): the mirror and the checks, no device behind them
static int iir_init(cmhip_iir_t *m, bool device)
{
    const cmhip_iir_desc_t &d = m->d;
    const size_t S = d.streams;
    m->ramp.init(S * d.sections);
    m->dirty = true;
    if (!device)
        return COOLMIC_ERROR_NONE;
    if (m->open("iir_new", d.device, d.hip_stream, S + iir_table_words(d, true)) ||
        m->array("iir_new", &m->d_state, S * d.channels * d.sections) || m->array("iir_new", &m->d_clips, S) ||
        m->array("iir_new", &m->d_overs, S))
        return COOLMIC_ERROR_GENERIC;
    return COOLMIC_ERROR_NONE;
}

static cmhip_iir_t *iir_new(const cmhip_iir_desc_t *d, bool device)
{
    if (!d) {
        fail(COOLMIC_ERROR_FAULT, "iir_new: NULL argument");
        return nullptr;
    }
    if (!iir_geometry_ok(d->streams, d->channels, d->sections, d->max_frames)) {
        fail(COOLMIC_ERROR_INVAL, "iir_new: streams, channels (1..16), sections (1..8) and max_frames (times channels below "
             "2^31) out of range");
        return nullptr;
    }
    return stage_new<cmhip_iir>("iir_new", [&](cmhip_iir_t *m) {
        m->d = *d;
        return iir_init(m, device);
    });
}

extern "C" cmhip_iir_t *cmhip_iir_new(const cmhip_iir_desc_t *d) { return iir_new(d, true); }

// test hook: an object with its mirror and every check but no device behind it, for the refusals and the mirror's
// answers on a machine without a GPU; a run that would launch is refused
extern "C" cmhip_iir_t *cmhip_test_iir_new_dry(const cmhip_iir_desc_t *d) { return iir_new(d, false); }

extern "C" void *cmhip_iir_hip_stream(cmhip_iir_t *m) { return m ? (void *)m->stream : nullptr; }

extern "C" int cmhip_iir_sync(cmhip_iir_t *m) { return stage_sync(m, "iir_sync"); }

extern "C" int cmhip_iir_set(cmhip_iir_t *m, long stream, unsigned int section, const cmhip_iir_section_t *c)
{
    if (!c)
        return fail(COOLMIC_ERROR_FAULT, "iir_set: NULL argument");
    StreamRange sr;
    const int rc = stage_streams(m, "iir_set", stream, &sr);
    if (rc)
        return rc;
    if (section >= m->d.sections)
        return fail(COOLMIC_ERROR_INVAL, "iir_set: section %u of %u", section, m->d.sections);
    const IirSec q = iir_from(c);
    if (!iir_section_ok(q))
        return fail(COOLMIC_ERROR_INVAL, "iir_set: every |c| <= 2^28, |a2| < 2^26 and |a1| < 2^26 + a2 are required");
    for (size_t s = sr.lo; s < (size_t)sr.lo + sr.n; s++)
        m->ramp.cancel(s * m->d.sections + section, q);
    m->dirty = true;
    return COOLMIC_ERROR_NONE;
}

extern "C" int cmhip_iir_ramp(cmhip_iir_t *m, long stream, unsigned int section, const cmhip_iir_section_t *target,
                              uint32_t ramp_frames)
{
    if (!target)
        return fail(COOLMIC_ERROR_FAULT, "iir_ramp: NULL argument");
    StreamRange sr;
    const int rc = stage_streams(m, "iir_ramp", stream, &sr);
    if (rc)
        return rc;
    if (section >= m->d.sections)
        return fail(COOLMIC_ERROR_INVAL, "iir_ramp: section %u of %u", section, m->d.sections);
    if (ramp_frames > IIR_RAMP_MAX)
        return fail(COOLMIC_ERROR_INVAL, "iir_ramp: %u frames, at most %u", ramp_frames, IIR_RAMP_MAX);
    const IirSec q = iir_from(target);
    if (!iir_section_ok(q))
        return fail(COOLMIC_ERROR_INVAL, "iir_ramp: every |c| <= 2^28, |a2| < 2^26 and |a1| < 2^26 + a2 are required");
    for (size_t s = sr.lo; s < (size_t)sr.lo + sr.n; s++) {
        const size_t i = s * m->d.sections + section;
        if (ramp_frames < 2)
            m->ramp.cancel(i, q);                    // a step: cmhip_iir_set
        else
            m->ramp.start(i, q, ramp_frames);
    }
    m->dirty = true;
    return COOLMIC_ERROR_NONE;
}

extern "C" int cmhip_iir_ramp_state(const cmhip_iir_t *m, unsigned int stream, unsigned int section, uint32_t *done,
                                    uint32_t *ramp_frames)
{
    if (!m)
        return fail(COOLMIC_ERROR_FAULT, "iir_ramp_state: NULL argument");
    if (stream >= m->d.streams || section >= m->d.sections)
        return fail(COOLMIC_ERROR_INVAL, "iir_ramp_state: stream %u, section %u out of range", stream, section);
    const IirRampEntry &e = m->ramp.e[(size_t)stream * m->d.sections + section];
    if (done)
        *done = e.done;
    if (ramp_frames)
        *ramp_frames = e.R;
    return COOLMIC_ERROR_NONE;
}

// c(p) between two sections; an end's coefficient outside +-2^28, which no valid section has, counts as the bound
extern "C" void cmhip_iir_ramp_section(const cmhip_iir_section_t *c0, const cmhip_iir_section_t *c1, uint32_t p,
                                       cmhip_iir_section_t *out)
{
    if (!c0 || !c1 || !out)
        return;
    IirSec e[2] = {iir_from(c0), iir_from(c1)};
    for (IirSec &c : e)
        for (int32_t *v : {&c.b0, &c.b1, &c.b2, &c.a1, &c.a2})
            *v = *v < -IIR_COEF_MAX ? -IIR_COEF_MAX : *v > IIR_COEF_MAX ? IIR_COEF_MAX : *v;
    const IirSec c = iir_ramp_section(e[0], e[1], p);
    memcpy(out, &c, sizeof(c));
}

extern "C" int cmhip_iir_get(const cmhip_iir_t *m, unsigned int stream, unsigned int section, cmhip_iir_section_t *c)
{
    if (!m || !c)
        return fail(COOLMIC_ERROR_FAULT, "iir_get: NULL argument");
    if (stream >= m->d.streams || section >= m->d.sections)
        return fail(COOLMIC_ERROR_INVAL, "iir_get: stream %u, section %u out of range", stream, section);
    const IirSec now = m->ramp.now((size_t)stream * m->d.sections + section);
    memcpy(c, &now, sizeof(*c));
    return COOLMIC_ERROR_NONE;
}

extern "C" int cmhip_iir_run(cmhip_iir_t *m, const void *in, size_t in_stride, size_t frames,
                             const uint32_t *frames_per_stream, void *out, size_t out_stride)
{
    if (!m)
        return fail(COOLMIC_ERROR_FAULT, "iir_run: NULL argument");
    const unsigned S = m->d.streams, C = m->d.channels;
    const StageRun r = {in, out, in_stride, out_stride, frames, m->d.max_frames, frames_per_stream, S, S, C, frames, C,
                        STAGE_APART};
    int rc;
    if (!stage_run_begin(m, "iir_run", r, &rc))
        return rc;
    // nothing was touched so far; from here on the run happens
    // the run's counts and, behind a set or while a section ramps, the coefficient table behind them
    uint32_t *block;
    HIP_TRY(m->counts.take(&block));
    for (unsigned s = 0; s < S; s++)
        block[s] = stage_count(frames_per_stream, s, frames);
    const bool ramp = m->ramp.any();
    const size_t words = ramp || m->dirty ? iir_table_words(m->d, ramp) : 0;
    if (ramp) {
        memcpy(block + S, m->ramp.e.data(), words * sizeof(uint32_t));
    } else if (words) {
        IirSec *table = (IirSec *)(block + S);
        for (size_t i = 0; i < m->ramp.e.size(); i++)
            table[i] = m->ramp.e[i].c1;
    }
    HIP_TRY(m->counts.send(m->d_counts, S + words, m->stream));
    // the mirror behind this run: every section by its stream's count; what the device holds is a ramp table then
    m->dirty = ramp;
    if (ramp)
        for (unsigned s = 0; s < S; s++)
            for (unsigned k = 0; k < m->d.sections; k++)
                m->ramp.advance((size_t)s * m->d.sections + k, block[s]);
    IirArgs a;
    memset(&a, 0, sizeof(a));
    a.in = (const int16_t *)in;
    a.out = (int16_t *)out;
    a.counts = m->d_counts;
    a.coef = (const int32_t *)(m->d_counts + S);
    a.state = m->d_state;
    a.clips = m->d_clips;
    a.overs = m->d_overs;
    a.in_stride = in_stride;
    a.out_stride = out_stride;
    a.streams = S;
    a.channels = C;
    a.sections = m->d.sections;
    return stage_launched("iir_run", launch_iir(a, (uint32_t)frames, ramp, m->stream));
}

extern "C" int cmhip_iir_reset(cmhip_iir_t *m, long stream)
{
    StreamRange sr;
    const int rc = stage_streams(m, "iir_reset", stream, &sr);
    if (rc || !m->opened)
        return rc;
    HIP_TRY(hipSetDevice(m->d.device));
    const size_t per = (size_t)m->d.channels * m->d.sections;            // a stream's sections, all rows
    HIP_TRY(hipMemsetAsync(m->d_state + (size_t)sr.lo * per, 0, (size_t)sr.n * per * sizeof(IirState), m->stream));
    return COOLMIC_ERROR_NONE;
}

extern "C" int cmhip_iir_state(cmhip_iir_t *m, uint64_t *clips, uint64_t *overs, int clear)
{
    if (!m)
        return fail(COOLMIC_ERROR_FAULT, "iir_state: NULL argument");
    const size_t bytes = (size_t)m->d.streams * sizeof(uint64_t);
    const int rc = stage_read(m, clips, m->d_clips, bytes, clear != 0);
    return rc ? rc : stage_read(m, overs, m->d_overs, bytes, clear != 0);
}

// test hook: the rows' sections as the device holds them, int32 [S * C][N][5] (u1, u2, v1, v2, e); synchronous
extern "C" int cmhip_test_iir_rows(cmhip_iir_t *m, int32_t *rows)
{
    if (!m || !rows)
        return fail(COOLMIC_ERROR_FAULT, "iir_rows: NULL argument");
    return stage_read(m, rows, m->d_state, (size_t)m->d.streams * m->d.channels * m->d.sections * sizeof(IirState), false);
}
