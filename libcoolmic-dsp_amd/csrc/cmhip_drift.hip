// cmhip_drift.hip -- clock-drift compensation on the host side (include/coolmic_hip.h, "clock-drift compensation"): the
// object beside the batch, its validation, the host's mirror of every stream's step, position and totals, the design
// of the table, the servo, and the launch of k_drift.hip's kernel.
//
// Device state of a drift stage: the table in the kernel's form (csrc/drift_plan.h) and the streams' history, int16
// [2][S][C][T-1] in two slots (HistoryPair).  Step, position and totals live in the host's mirror: the host sees every
// run's counts, every set, seek and reset, so a run's records travel to the device with the run, through the counts
// ring, and a run's output counts are known before the call returns, without a device wait.  A set or a seek changes
// the mirror alone and is ordered with the runs by the order of the calls.
#include "cmhip_engine.h"
#include "design_window.h"

#include <math.h>
#include <string.h>

constexpr uint64_t DRIFT_MAX_SAMPLES = 1ull << 31;   // per slot and run: the kernels index a slot in 32 bits
constexpr unsigned DRIFT_DEFAULT_PHI = 7, DRIFT_DEFAULT_T = 32;

static_assert(sizeof(cmhip_drift_servo_t) == sizeof(DriftServo) &&
                  offsetof(cmhip_drift_servo_t, clamped) == offsetof(DriftServo, clamped) &&
                  offsetof(cmhip_drift_servo_t, limit) == offsetof(DriftServo, limit),
              "cmhip_drift_servo_t is DriftServo");
static_assert(CMHIP_DRIFT_DELTA_MAX == DRIFT_DELTA_MAX, "one limit");

struct cmhip_drift : StageBase {
    cmhip_drift_desc_t d;
    unsigned phi, T;
    size_t max_out;                    // drift_out_frames(0, -2^24, max_in_frames)
    uint32_t *d_table;
    HistoryPair hist;                  // [2][S][C * (T-1)]
    DriftMirror mirror;
};

extern "C" uint32_t cmhip_drift_out_frames(uint64_t pos, int32_t delta, uint32_t frames)
{
    return drift_out_frames(pos, delta, frames);
}

extern "C" int32_t cmhip_drift_ppm(double ppm)
{
    if (isnan(ppm))
        return 0;
    const double v = rint(ppm * 4294967296.0 / 1e6);
    return v < -(double)DRIFT_DELTA_MAX ? -DRIFT_DELTA_MAX : v > (double)DRIFT_DELTA_MAX ? DRIFT_DELTA_MAX : (int32_t)v;
}

extern "C" double cmhip_drift_to_ppm(int32_t delta) { return (double)delta * 1e6 / 4294967296.0; }

extern "C" int cmhip_drift_servo_init(cmhip_drift_servo_t *servo, uint32_t target_frames, unsigned kp_log2,
                                      unsigned ki_log2, int32_t limit)
{
    if (!servo)
        return fail(COOLMIC_ERROR_FAULT, "drift_servo_init: NULL argument");
    DriftServo v;
    if (!drift_servo_init(&v, target_frames, kp_log2, ki_log2, limit))
        return fail(COOLMIC_ERROR_INVAL, "drift_servo_init: a target below 2^31, shifts of 0..%u and a limit of 1..2^24 are "
                    "required", DRIFT_SERVO_SHIFT_MAX);
    memcpy(servo, &v, sizeof(v));
    return COOLMIC_ERROR_NONE;
}

extern "C" int32_t cmhip_drift_servo_step(cmhip_drift_servo_t *servo, int64_t fill_frames)
{
    return servo ? drift_servo_step(reinterpret_cast<DriftServo *>(servo), fill_frames) : 0;
}

extern "C" void cmhip_drift_servo_reset(cmhip_drift_servo_t *servo)
{
    if (servo)
        drift_servo_reset(reinterpret_cast<DriftServo *>(servo));
}

static int drift_table_refusal(const char *who, unsigned phi, unsigned T, const int16_t *h)
{
    uint32_t where = 0;
    switch (drift_table_check(phi, T, h, &where)) {
    case DRIFT_TABLE_OK: return COOLMIC_ERROR_NONE;
    case DRIFT_TABLE_GEOMETRY:
        return fail(COOLMIC_ERROR_INVAL, "%s: phase_log2 = %u, taps = %u: %u..%u and an even count in %u..%u are required", who,
                    phi, T, DRIFT_PHI_MIN, DRIFT_PHI_MAX, DRIFT_T_MIN, DRIFT_T_MAX);
    case DRIFT_TABLE_FIRST: return fail(COOLMIC_ERROR_INVAL, "%s: H[0][0] must be 0", who);
    case DRIFT_TABLE_SUM: return fail(COOLMIC_ERROR_INVAL, "%s: row %u has sum |h| above 65535", who, where);
    }
    return fail(COOLMIC_ERROR_GENERIC, "%s: unknown error", who);
}

// (the body of cmhip_drift_design: its vector may throw)
static int drift_design(unsigned phi, unsigned T, int16_t *h, size_t cap)
{
    if (!h)
        return fail(COOLMIC_ERROR_FAULT, "drift_design: NULL argument");
    if (!drift_geometry_ok(phi, T))
        return fail(COOLMIC_ERROR_INVAL, "drift_design: phase_log2 = %u, taps = %u: %u..%u and an even count in %u..%u are "
                    "required", phi, T, DRIFT_PHI_MIN, DRIFT_PHI_MAX, DRIFT_T_MIN, DRIFT_T_MAX);
    const unsigned P = 1u << phi;
    const size_t N = (size_t)P * T;
    if (cap < N)
        return fail(COOLMIC_ERROR_INVAL, "drift_design: room for %zu entries, the table has %zu", cap, N);
    const double fc = 0.92 * 0.5, i0b = design_i0(DESIGN_BETA);
    std::vector<int16_t> tab(N);
    for (unsigned p = 0; p < P; p++) {
        double g[DRIFT_T_MAX], sum = 0.0;
        for (unsigned k = 0; k < T; k++) {
            const double x = (double)k + (double)p / (double)P - (double)T / 2.0;
            g[k] = design_tap(x, (double)T / 2.0, fc, i0b);                  // the resampler's window and sinc
            if (p == 0 && k == 0)
                g[k] = 0.0;
            sum += g[k];
        }
        long isum = 0, q[DRIFT_T_MAX];
        unsigned big = 0;
        for (unsigned k = 0; k < T; k++) {
            q[k] = (long)rint(g[k] / sum * 16384.0);
            isum += q[k];
            if (labs(q[k]) > labs(q[big]))
                big = k;                                 // the first tap of largest magnitude
        }
        q[big] += 16384 - isum;
        for (unsigned k = 0; k < T; k++) {
            if (q[k] < -32768 || q[k] > 32767)
                return fail(COOLMIC_ERROR_GENERIC, "drift_design: a coefficient left int16");
            tab[(size_t)p * T + k] = (int16_t)q[k];
        }
    }
    if (drift_table_refusal("drift_design", phi, T, tab.data()))
        return COOLMIC_ERROR_GENERIC;
    memcpy(h, tab.data(), N * sizeof(int16_t));
    return COOLMIC_ERROR_NONE;
}

extern "C" int cmhip_drift_design(unsigned phase_log2, unsigned taps, int16_t *h, size_t cap)
{
    return stage_guard("drift_design", [&] { return drift_design(phase_log2, taps, h, cap); });
}

// device false (cmhip_test_drift_new_dry): the mirror and the checks, no device behind them
static int drift_init(cmhip_drift_t *m, const int16_t *h, bool device)
{
    const cmhip_drift_desc_t &d = m->d;
    const size_t S = d.streams;
    m->mirror.init(S);
    if (!device)
        return COOLMIC_ERROR_NONE;
    std::vector<uint32_t> tab(drift_table_words(m->phi, m->T));
    drift_compile(m->phi, m->T, h, tab.data());
    if (m->open("drift_new", d.device, d.hip_stream, S * DRIFT_REC) || m->alloc("drift_new", &m->d_table, tab.size()) ||
        m->hist.init(*m, "drift_new", S, (size_t)d.channels * (m->T - 1)))
        return COOLMIC_ERROR_GENERIC;
    HIP_TRY(hipMemcpy(m->d_table, tab.data(), tab.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    return COOLMIC_ERROR_NONE;
}

static cmhip_drift_t *drift_new_table(const cmhip_drift_desc_t *d, unsigned phi, unsigned T, const int16_t *h, bool device)
{
    if (!d || !h) {
        fail(COOLMIC_ERROR_FAULT, "drift_new: NULL argument");
        return nullptr;
    }
    if (d->streams == 0 || d->channels == 0 || d->channels > MAX_CH || d->max_in_frames == 0) {
        fail(COOLMIC_ERROR_INVAL, "drift_new: streams, channels (1..16) and max_in_frames must be positive");
        return nullptr;
    }
    if (drift_table_refusal("drift_new", phi, T, h))
        return nullptr;
    if ((uint64_t)d->max_in_frames * d->channels > DRIFT_MAX_SAMPLES ||
        (uint64_t)drift_out_frames(0, -DRIFT_DELTA_MAX, (uint32_t)d->max_in_frames) * d->channels > DRIFT_MAX_SAMPLES) {
        fail(COOLMIC_ERROR_INVAL, "drift_new: max_in_frames %zu: a slot of a run would pass 2^31 samples", d->max_in_frames);
        return nullptr;
    }
    return stage_new<cmhip_drift>("drift_new", [&](cmhip_drift_t *m) {
        m->d = *d;
        m->phi = phi;
        m->T = T;
        m->max_out = drift_out_frames(0, -DRIFT_DELTA_MAX, (uint32_t)d->max_in_frames);
        return drift_init(m, h, device);
    });
}

static cmhip_drift_t *drift_new(const cmhip_drift_desc_t *d, bool device)
{
    cmhip_drift_t *m = nullptr;
    (void)stage_guard("drift_new", [&] {
        std::vector<int16_t> h((size_t)DRIFT_DEFAULT_T << DRIFT_DEFAULT_PHI);
        if (!drift_design(DRIFT_DEFAULT_PHI, DRIFT_DEFAULT_T, h.data(), h.size()))
            m = drift_new_table(d, DRIFT_DEFAULT_PHI, DRIFT_DEFAULT_T, h.data(), device);
        return 0;
    });
    return m;
}

extern "C" void cmhip_drift_free(cmhip_drift_t *m) { stage_free(m); }

extern "C" cmhip_drift_t *cmhip_drift_new_table(const cmhip_drift_desc_t *d, unsigned phase_log2, unsigned taps,
                                                const int16_t *h)
{
    return drift_new_table(d, phase_log2, taps, h, true);
}

extern "C" cmhip_drift_t *cmhip_drift_new(const cmhip_drift_desc_t *d) { return drift_new(d, true); }

// test hook: an object with its mirror and every check but no device behind it (h NULL: the designed default), for
// the refusals and the mirror's answers on a machine without a GPU; a run that would launch is refused
extern "C" cmhip_drift_t *cmhip_test_drift_new_dry(const cmhip_drift_desc_t *d, unsigned phase_log2, unsigned taps,
                                                   const int16_t *h)
{
    return h ? drift_new_table(d, phase_log2, taps, h, false) : drift_new(d, false);
}

extern "C" int cmhip_drift_geometry(const cmhip_drift_t *m, unsigned *phase_log2, unsigned *taps)
{
    if (!m)
        return fail(COOLMIC_ERROR_FAULT, "drift_geometry: NULL argument");
    if (phase_log2)
        *phase_log2 = m->phi;
    if (taps)
        *taps = m->T;
    return COOLMIC_ERROR_NONE;
}

extern "C" size_t cmhip_drift_max_out_frames(const cmhip_drift_t *m) { return m ? m->max_out : 0; }
extern "C" void *cmhip_drift_hip_stream(cmhip_drift_t *m) { return m ? (void *)m->stream : nullptr; }

extern "C" int cmhip_drift_sync(cmhip_drift_t *m) { return stage_sync(m, "drift_sync"); }

extern "C" int cmhip_drift_set(cmhip_drift_t *m, long stream, int32_t delta)
{
    StreamRange sr;
    const int rc = stage_streams(m, "drift_set", stream, &sr);
    if (rc)
        return rc;
    if (!drift_delta_ok(delta))
        return fail(COOLMIC_ERROR_INVAL, "drift_set: delta %d outside +-2^24", (int)delta);
    for (size_t s = sr.lo; s < (size_t)sr.lo + sr.n; s++)
        m->mirror.delta[s] = delta;
    return COOLMIC_ERROR_NONE;
}

extern "C" int cmhip_drift_seek(cmhip_drift_t *m, long stream, uint64_t frac)
{
    StreamRange sr;
    const int rc = stage_streams(m, "drift_seek", stream, &sr);
    if (rc)
        return rc;
    if (frac >= DRIFT_ONE)
        return fail(COOLMIC_ERROR_INVAL, "drift_seek: a fraction below 2^32 is required");
    for (size_t s = sr.lo; s < (size_t)sr.lo + sr.n; s++)
        m->mirror.pos[s] = frac;
    return COOLMIC_ERROR_NONE;
}

extern "C" int cmhip_drift_get(const cmhip_drift_t *m, unsigned stream, int32_t *delta, uint64_t *pos, uint64_t *in_total,
                               uint64_t *out_total)
{
    if (!m)
        return fail(COOLMIC_ERROR_FAULT, "drift_get: NULL argument");
    if (stream >= m->d.streams)
        return fail(COOLMIC_ERROR_INVAL, "drift_get: stream %u out of range", stream);
    if (delta)
        *delta = m->mirror.delta[stream];
    if (pos)
        *pos = m->mirror.pos[stream];
    if (in_total)
        *in_total = m->mirror.in_total[stream];
    if (out_total)
        *out_total = m->mirror.out_total[stream];
    return COOLMIC_ERROR_NONE;
}

// the mirror's part of a run: every stream's output count, and the mirror moved on
static void drift_advance(cmhip_drift_t *m, size_t frames, const uint32_t *frames_per_stream, uint32_t *out_frames)
{
    for (unsigned s = 0; s < m->d.streams; s++) {
        const uint32_t k = m->mirror.advance(s, stage_count(frames_per_stream, s, frames));
        if (out_frames)
            out_frames[s] = k;
    }
}

// test hook: the mirror's part of a run alone (frames and counts as cmhip_drift_run takes them, unchecked but for
// a count above frames), for the mirror's answers on a machine without a GPU
extern "C" int cmhip_test_drift_advance(cmhip_drift_t *m, size_t frames, const uint32_t *frames_per_stream,
                                        uint32_t *out_frames)
{
    if (!m)
        return fail(COOLMIC_ERROR_FAULT, "drift_advance: NULL argument");
    if (frames > m->d.max_in_frames)
        return fail(COOLMIC_ERROR_INVAL, "drift_advance: %zu frames above the object's %zu", frames, m->d.max_in_frames);
    for (unsigned s = 0; s < m->d.streams; s++)
        if (stage_count(frames_per_stream, s, frames) > frames)
            return fail(COOLMIC_ERROR_INVAL, "drift_advance: frames_per_stream[%u] above frames", s);
    drift_advance(m, frames, frames_per_stream, out_frames);
    return COOLMIC_ERROR_NONE;
}

// test hook: the plan of a run that gives its longest stream out_frames frames (host logic, needs no GPU)
extern "C" void cmhip_test_plan_drift(uint32_t streams, uint32_t channels, uint32_t phase_log2, uint32_t taps,
                                      uint32_t out_frames, DriftPlan *plan)
{
    if (plan)
        *plan = plan_drift(streams, channels, phase_log2, taps, out_frames);
}

extern "C" int cmhip_drift_run(cmhip_drift_t *m, const void *in, size_t in_stride, size_t frames,
                               const uint32_t *frames_per_stream, void *out, size_t out_stride, uint32_t *out_frames)
{
    if (!m)
        return fail(COOLMIC_ERROR_FAULT, "drift_run: NULL argument");
    const unsigned S = m->d.streams, C = m->d.channels;
    // what the run gives its longest stream (pure arithmetic on counts the check below has yet to judge)
    uint32_t most = 0;
    for (unsigned s = 0; s < S; s++) {
        const uint32_t k = m->mirror.out_frames(s, stage_count(frames_per_stream, s, frames));
        if (k > most)
            most = k;
    }
    const StageRun run = {in, out, in_stride, out_stride, frames, m->d.max_in_frames, frames_per_stream, S, S, C, most, C,
                          STAGE_NOT_IN_PLACE};
    int rc;
    const bool go = stage_run_begin(m, "drift_run", run, &rc);
    if (rc)
        return rc;
    if (go) {
        if (plan_drift(S, C, m->phi, m->T, most ? most : 1u).err)
            return fail(COOLMIC_ERROR_INVAL, "drift_run: %u streams of %u outputs: the grid would reach 2^31 workgroups", S,
                        most);
        // nothing was touched so far; from here on the run happens
        uint32_t *block;
        HIP_TRY(m->counts.take(&block));
        for (unsigned s = 0; s < S; s++)
            m->mirror.record(s, stage_count(frames_per_stream, s, frames), block + (size_t)s * DRIFT_REC);
        HIP_TRY(m->counts.send(m->d_counts, (size_t)S * DRIFT_REC, m->stream));
        DriftArgs a;
        memset(&a, 0, sizeof(a));
        a.in = (const int16_t *)in;
        a.out = (int16_t *)out;
        a.rec = m->d_counts;
        a.table = m->d_table;
        a.hist = m->hist.d;
        a.in_stride = in_stride;
        a.out_stride = out_stride;
        a.streams = S;
        a.channels = C;
        a.parity = m->hist.parity();
        a.phi = m->phi;
        a.T = m->T;
        // (a run that gives no stream an output still moves the history: one workgroup per stream)
        rc = stage_launched("drift_run", launch_drift(a, most ? most : 1u, m->stream));
        if (rc)
            return rc;
        m->hist.flip();                      // the kernel wrote the other slots
    }
    drift_advance(m, frames, frames_per_stream, out_frames);
    return COOLMIC_ERROR_NONE;
}

extern "C" int cmhip_drift_reset(cmhip_drift_t *m, long stream)
{
    StreamRange sr;
    const int rc = stage_streams(m, "drift_reset", stream, &sr);
    if (rc)
        return rc;
    if (m->opened) {
        HIP_TRY(hipSetDevice(m->d.device));
        HIP_TRY(m->hist.reset(sr.lo, sr.n, m->stream));
    }
    for (size_t s = sr.lo; s < (size_t)sr.lo + sr.n; s++)
        m->mirror.reset(s);
    return COOLMIC_ERROR_NONE;
}
