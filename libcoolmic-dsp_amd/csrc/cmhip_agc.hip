// cmhip_agc.hip -- the leveller on the host side (include/coolmic_hip.h, "leveller"): the object beside the batch, its
// validation, the host's mirror of every stream's position and parameters, the design of parameters from a law in dB,
// and the launch of k_agc.hip's kernels.
//
// Device state of a leveller: per stream the open window's sums, the two gain nodes in force and the last level
// (AgcState), and the clip counter; per run the table of sums [S][NW][C] and the gain nodes [S][NW + 1].  Positions and
// parameters live in the host's mirror: the host sees every run's counts and every set, so a run's records -- count,
// position and parameters per stream -- travel to the device with the run, through the counts ring.  A set or a reset
// therefore changes the mirror alone and is ordered with the runs by the order of the calls: a stream whose record says
// position 0 starts afresh from `initial`.
#include "cmhip_engine.h"

#include <math.h>
#include <string.h>

static_assert(sizeof(cmhip_agc_params_t) == sizeof(AgcParams) && sizeof(AgcParams) == 14, "cmhip_agc_params_t is AgcParams");
static_assert(offsetof(cmhip_agc_params_t, initial) == offsetof(AgcParams, initial), "cmhip_agc_params_t is AgcParams");

struct cmhip_agc : StageBase {
    cmhip_agc_desc_t d;
    uint32_t nw;                       // windows per stream in the two tables
    unsigned long long *d_table;       // [S][nw][C]
    uint32_t *d_nodes;                 // [S][nw + 1]
    AgcState *d_state;                 // [S]
    unsigned long long *d_clips;       // [S]
    AgcMirror mirror;
};

static const AgcParams AGC_DEFAULT = {3277, 33, AGC_UNITY, AGC_UNITY, 0, 0, AGC_UNITY};

static AgcParams agc_from(const cmhip_agc_params_t *p)
{
    AgcParams q;
    memcpy(&q, p, sizeof(q));
    return q;
}

extern "C" int cmhip_agc_check(unsigned int window_log2, const cmhip_agc_params_t *p)
{
    if (!agc_window_ok(window_log2))
        return fail(COOLMIC_ERROR_INVAL, "agc_check: window_log2 %u outside %u..%u", window_log2, AGC_W_MIN, AGC_W_MAX);
    if (p && !agc_params_ok(agc_from(p)))
        return fail(COOLMIC_ERROR_INVAL,
                    "agc_check: target 1..32767, gate 0..32767 and 1 <= gain_min <= initial <= gain_max are required");
    return COOLMIC_ERROR_NONE;
}

// rint(v) clamped to lo..hi (v finite)
static uint16_t agc_round(double v, double lo, double hi)
{
    v = rint(v);
    return (uint16_t)(v < lo ? lo : v > hi ? hi : v);
}

extern "C" int cmhip_agc_design(const cmhip_agc_law_desc_t *law, cmhip_agc_params_t *p)
{
    if (!law || !p)
        return fail(COOLMIC_ERROR_FAULT, "agc_design: NULL argument");
    const double in[9] = {law->rate, law->window_log2, law->target_db, law->gate_db, law->max_gain_db, law->min_gain_db,
                          law->initial_gain_db, law->rise_db_per_s, law->fall_db_per_s};
    for (double v : in)
        if (!isfinite(v))
            return fail(COOLMIC_ERROR_INVAL, "agc_design: a value is not finite");
    if (!(law->rate > 0.0) || law->window_log2 != rint(law->window_log2) || law->window_log2 < (double)AGC_W_MIN ||
        law->window_log2 > (double)AGC_W_MAX)
        return fail(COOLMIC_ERROR_INVAL, "agc_design: the rate must be positive and window_log2 an integer in %u..%u",
                    AGC_W_MIN, AGC_W_MAX);
    if (law->rise_db_per_s < 0.0 || law->fall_db_per_s < 0.0 || law->min_gain_db > law->max_gain_db)
        return fail(COOLMIC_ERROR_INVAL, "agc_design: negative rates of change, or min_gain_db above max_gain_db");
    const double window_s = ldexp(1.0, (int)law->window_log2) / law->rate;
    AgcParams q;
    q.target = agc_round(32768.0 * pow(10.0, law->target_db / 20.0), 1.0, 32767.0);
    q.gate = agc_round(32768.0 * pow(10.0, law->gate_db / 20.0), 0.0, 32767.0);
    q.gain_max = agc_round(4096.0 * pow(10.0, law->max_gain_db / 20.0), 1.0, 65535.0);
    q.gain_min = agc_round(4096.0 * pow(10.0, law->min_gain_db / 20.0), 1.0, 65535.0);
    q.initial = agc_round(4096.0 * pow(10.0, law->initial_gain_db / 20.0), (double)q.gain_min, (double)q.gain_max);
    const double up = (pow(10.0, law->rise_db_per_s * window_s / 20.0) - 1.0) * 65536.0;
    const double down = (1.0 - pow(10.0, -law->fall_db_per_s * window_s / 20.0)) * 65536.0;
    q.rise = agc_round(up < 65535.0 ? up : 65535.0, 0.0, 65535.0);          // (an overflow to infinity included)
    q.fall = agc_round(down, 0.0, 65535.0);
    memcpy(p, &q, sizeof(q));
    return COOLMIC_ERROR_NONE;
}

// test hook: the header's step(A, L) as code
extern "C" uint32_t cmhip_test_agc_step(uint32_t A, uint32_t L, const cmhip_agc_params_t *p)
{
    return p ? agc_step(A, L, agc_from(p)) : 0u;
}

extern "C" void cmhip_agc_free(cmhip_agc_t *m) { stage_free(m); }

// device false (cmhip_test_agc_new_dry): the mirror and the checks, no device behind them
static int agc_init(cmhip_agc_t *m, bool device)
{
    const cmhip_agc_desc_t &d = m->d;
    const size_t S = d.streams;
    m->mirror.init(S, AGC_DEFAULT);
    if (!device)
        return COOLMIC_ERROR_NONE;
    if (m->open("agc_new", d.device, d.hip_stream, S * AGC_REC) ||
        m->array("agc_new", &m->d_table, S * m->nw * d.channels) ||
        m->array("agc_new", &m->d_nodes, S * ((size_t)m->nw + 1u)) || m->array("agc_new", &m->d_state, S) ||
        m->array("agc_new", &m->d_clips, S))
        return COOLMIC_ERROR_GENERIC;
    return COOLMIC_ERROR_NONE;
}

static cmhip_agc_t *agc_new(const cmhip_agc_desc_t *d, bool device)
{
    if (!d) {
        fail(COOLMIC_ERROR_FAULT, "agc_new: NULL argument");
        return nullptr;
    }
    if (!agc_geometry_ok(d->streams, d->channels, d->window_log2, d->max_frames)) {
        fail(COOLMIC_ERROR_INVAL, "agc_new: streams, channels (1..16), window_log2 (%u..%u) and max_frames (times channels "
             "below 2^31) out of range", AGC_W_MIN, AGC_W_MAX);
        return nullptr;
    }
    return stage_new<cmhip_agc>("agc_new", [&](cmhip_agc_t *m) {
        m->d = *d;
        m->nw = agc_table_windows(d->max_frames, d->window_log2);
        return agc_init(m, device);
    });
}

extern "C" cmhip_agc_t *cmhip_agc_new(const cmhip_agc_desc_t *d) { return agc_new(d, true); }

// test hook: an object with its mirror and every check but no device behind it, for the refusals and the mirror's
// answers on a machine without a GPU; a run that would launch is refused
extern "C" cmhip_agc_t *cmhip_test_agc_new_dry(const cmhip_agc_desc_t *d) { return agc_new(d, false); }

extern "C" void *cmhip_agc_hip_stream(cmhip_agc_t *m) { return m ? (void *)m->stream : nullptr; }

extern "C" int cmhip_agc_sync(cmhip_agc_t *m) { return stage_sync(m, "agc_sync"); }

extern "C" int cmhip_agc_set(cmhip_agc_t *m, long stream, const cmhip_agc_params_t *p)
{
    if (!p)
        return fail(COOLMIC_ERROR_FAULT, "agc_set: NULL argument");
    StreamRange sr;
    const int rc = stage_streams(m, "agc_set", stream, &sr);
    if (rc)
        return rc;
    const AgcParams q = agc_from(p);
    if (!agc_params_ok(q))
        return fail(COOLMIC_ERROR_INVAL,
                    "agc_set: target 1..32767, gate 0..32767 and 1 <= gain_min <= initial <= gain_max are required");
    for (size_t s = sr.lo; s < (size_t)sr.lo + sr.n; s++)
        m->mirror.par[s] = q;
    return COOLMIC_ERROR_NONE;
}

extern "C" int cmhip_agc_get(const cmhip_agc_t *m, unsigned stream, cmhip_agc_params_t *p)
{
    if (!m || !p)
        return fail(COOLMIC_ERROR_FAULT, "agc_get: NULL argument");
    if (stream >= m->d.streams)
        return fail(COOLMIC_ERROR_INVAL, "agc_get: stream %u out of range", stream);
    memcpy(p, &m->mirror.par[stream], sizeof(*p));
    return COOLMIC_ERROR_NONE;
}

static int agc_run_on(cmhip_agc_t *m, const void *in, size_t in_stride, size_t frames, const uint32_t *frames_per_stream,
                      void *out, size_t out_stride, hipEvent_t *ev)
{
    if (!m)
        return fail(COOLMIC_ERROR_FAULT, "agc_run: NULL argument");
    const unsigned S = m->d.streams, C = m->d.channels;
    const StageRun r = {in, out, in_stride, out_stride, frames, m->d.max_frames, frames_per_stream, S, S, C, frames, C,
                        STAGE_APART};
    int rc;
    if (!stage_run_begin(m, "agc_run", r, &rc))
        return rc;
    if (plan_agc(S, C, m->d.window_log2, m->d.max_frames, (uint32_t)frames).err)
        return fail(COOLMIC_ERROR_INVAL, "agc_run: %u streams of %zu frames: the grid would reach 2^31 workgroups", S, frames);
    // nothing was touched so far; from here on the run happens
    // the run's records: the counts, and beside each the stream's position and parameters
    uint32_t *block;
    HIP_TRY(m->counts.take(&block));
    for (unsigned s = 0; s < S; s++)
        m->mirror.record(s, stage_count(frames_per_stream, s, frames), block + (size_t)s * AGC_REC);
    HIP_TRY(m->counts.send(m->d_counts, (size_t)S * AGC_REC, m->stream));
    AgcArgs a;
    memset(&a, 0, sizeof(a));
    a.in = (const int16_t *)in;
    a.out = (int16_t *)out;
    a.rec = m->d_counts;
    a.table = m->d_table;
    a.nodes = m->d_nodes;
    a.state = m->d_state;
    a.clips = m->d_clips;
    a.in_stride = in_stride;
    a.out_stride = out_stride;
    a.streams = S;
    a.channels = C;
    a.w = m->d.window_log2;
    rc = stage_launched("agc_run", launch_agc(a, m->d.max_frames, (uint32_t)frames, m->stream, ev));
    for (unsigned s = 0; s < S && !rc; s++)
        m->mirror.pos[s] += stage_count(frames_per_stream, s, frames);
    return rc;
}

extern "C" int cmhip_agc_run(cmhip_agc_t *m, const void *in, size_t in_stride, size_t frames,
                             const uint32_t *frames_per_stream, void *out, size_t out_stride)
{
    return agc_run_on(m, in, in_stride, frames, frames_per_stream, out, out_stride, nullptr);
}

// test hook: cmhip_agc_run with four of the caller's events (hipEvent_t [4]) recorded on the object's stream in front
// of, between and behind the three launches, so that tools/bench_agc.py can time each kernel by itself
extern "C" int cmhip_test_agc_run_events(cmhip_agc_t *m, const void *in, size_t in_stride, size_t frames,
                                         const uint32_t *frames_per_stream, void *out, size_t out_stride, void **events)
{
    if (!events)
        return fail(COOLMIC_ERROR_FAULT, "agc_run_events: NULL argument");
    return agc_run_on(m, in, in_stride, frames, frames_per_stream, out, out_stride, (hipEvent_t *)events);
}

extern "C" int cmhip_agc_reset(cmhip_agc_t *m, long stream)
{
    StreamRange sr;
    const int rc = stage_streams(m, "agc_reset", stream, &sr);
    if (rc)
        return rc;
    for (size_t s = sr.lo; s < (size_t)sr.lo + sr.n; s++)
        m->mirror.pos[s] = 0;                        // the next record says so, and k_agc_step starts afresh
    return COOLMIC_ERROR_NONE;
}

extern "C" int cmhip_agc_state(cmhip_agc_t *m, uint32_t *gain, uint32_t *level, uint64_t *clips, int clear_clips)
{
    if (!m)
        return fail(COOLMIC_ERROR_FAULT, "agc_state: NULL argument");
    return stage_guard("agc_state", [&] {
        const size_t S = m->d.streams;
        std::vector<AgcState> st(S);
        if (stage_read(m, st.data(), m->d_state, S * sizeof(AgcState), false) ||
            stage_read(m, clips, m->d_clips, S * sizeof(uint64_t), clear_clips != 0))
            return COOLMIC_ERROR_GENERIC;
        for (size_t s = 0; s < S; s++) {
            const bool fresh = !m->opened || m->mirror.pos[s] == 0;  // before frame 0: what the device holds is stale
            if (gain)
                gain[s] = fresh ? m->mirror.par[s].initial : st[s].a_hi;
            if (level)
                level[s] = fresh ? 0u : st[s].level;
        }
        return COOLMIC_ERROR_NONE;
    });
}
