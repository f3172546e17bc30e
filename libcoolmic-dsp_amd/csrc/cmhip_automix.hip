// cmhip_automix.hip -- the automixer on the host side (include/coolmic_hip.h, "automixer"): the object beside the batch,
// its validation, the host's mirror of every stream's position, parameters and group, the design of parameters from a
// law, and the launch of k_automix.hip's kernels.
//
// Device state of an automixer: per stream the open window's sums, P of the last complete window, the two gain nodes in
// force and the pending one (AutomixState); per run the table of sums [S][NW][C], the windows' P [S][NW], the groups'
// sums [S][NW] and the gain nodes [S][NW + 1].  Positions, parameters and groups live in the host's mirror
// (csrc/automix_plan.h): the host sees every run's counts, every set and every change of a group, so a run's records
// travel to the device with the run, through the counts ring -- twice over: as they are, and with count 0 for every
// stream in no group, which is what the energy pass reads.  A set, a set_group or a reset therefore changes the mirror
// alone and is ordered with the runs by the order of the calls: a stream whose record says position 0 starts afresh.
#include "cmhip_engine.h"

#include <math.h>
#include <string.h>

static_assert(sizeof(cmhip_automix_params_t) == sizeof(AutomixParams) && sizeof(AutomixParams) == 10,
              "cmhip_automix_params_t is AutomixParams");
static_assert(offsetof(cmhip_automix_params_t, initial) == offsetof(AutomixParams, initial),
              "cmhip_automix_params_t is AutomixParams");

struct cmhip_automix : StageBase {
    cmhip_automix_desc_t d;
    uint32_t nw;                       // windows per stream in the tables
    unsigned long long *d_table;       // [S][nw][C]
    unsigned long long *d_power;       // [S][nw]
    unsigned long long *d_gsum;        // [S][nw]
    uint32_t *d_nodes;                 // [S][nw + 1]
    AutomixState *d_state;             // [S]
    unsigned long long *d_clips;       // [S] what the shared apply body counts: g <= 4096, so it stays zero
    AutomixMirror mirror;
};

static const AutomixParams AUTOMIX_DEFAULT = {AUTOMIX_UNITY, 0, 0, 0, AUTOMIX_UNITY};
static const char AUTOMIX_RANGES[] = "weight, floor and initial 0..4096 and attack and release 0..8 are required";

static AutomixParams automix_from(const cmhip_automix_params_t *p)
{
    AutomixParams q;
    memcpy(&q, p, sizeof(q));
    return q;
}

extern "C" int cmhip_automix_check(unsigned int window_log2, const cmhip_automix_params_t *p)
{
    if (!agc_window_ok(window_log2))
        return fail(COOLMIC_ERROR_INVAL, "automix_check: window_log2 %u outside %u..%u", window_log2, AGC_W_MIN, AGC_W_MAX);
    if (p && !automix_params_ok(automix_from(p)))
        return fail(COOLMIC_ERROR_INVAL, "automix_check: %s", AUTOMIX_RANGES);
    return COOLMIC_ERROR_NONE;
}

// rint(v) clamped to lo..hi (v not NaN)
static uint16_t automix_round(double v, double lo, double hi)
{
    v = rint(v);
    return (uint16_t)(v < lo ? lo : v > hi ? hi : v);
}

// the smoothing shift whose time constant, 2^sh windows, is nearest to ms
static uint16_t automix_shift(double ms, double rate, double W)
{
    return ms > 0.0 ? automix_round(log2(ms * rate / 1000.0 / W), 0.0, (double)AUTOMIX_SHIFT_MAX) : 0;
}

extern "C" int cmhip_automix_design(const cmhip_automix_law_desc_t *law, cmhip_automix_params_t *p)
{
    if (!law || !p)
        return fail(COOLMIC_ERROR_FAULT, "automix_design: NULL argument");
    const double in[7] = {law->rate, law->window_log2, law->weight_db, law->floor_db, law->initial_db, law->attack_ms,
                          law->release_ms};
    for (double v : in)
        if (!isfinite(v))
            return fail(COOLMIC_ERROR_INVAL, "automix_design: a value is not finite");
    if (!(law->rate > 0.0) || law->window_log2 != rint(law->window_log2) || law->window_log2 < (double)AGC_W_MIN ||
        law->window_log2 > (double)AGC_W_MAX)
        return fail(COOLMIC_ERROR_INVAL, "automix_design: the rate must be positive and window_log2 an integer in %u..%u",
                    AGC_W_MIN, AGC_W_MAX);
    if (law->weight_db > 0.0)
        return fail(COOLMIC_ERROR_INVAL, "automix_design: weight_db above 0");
    const double W = ldexp(1.0, (int)law->window_log2), unity = (double)AUTOMIX_UNITY;
    AutomixParams q;
    q.weight = automix_round(unity * pow(10.0, law->weight_db / 10.0), 0.0, unity);
    q.floor = automix_round(unity * pow(10.0, law->floor_db / 20.0), 0.0, unity);
    q.initial = automix_round(unity * pow(10.0, law->initial_db / 20.0), 0.0, unity);
    q.attack = automix_shift(law->attack_ms, law->rate, W);
    q.release = automix_shift(law->release_ms, law->rate, W);
    memcpy(p, &q, sizeof(q));
    return COOLMIC_ERROR_NONE;
}

// test hooks: the header's P and D updates as code
extern "C" uint64_t cmhip_test_automix_power(uint64_t P, uint32_t m, const cmhip_automix_params_t *p)
{
    return p ? automix_power(P, m, automix_from(p)) : 0u;
}

extern "C" uint32_t cmhip_test_automix_share(uint64_t P, uint64_t sum, uint32_t floor, uint32_t D_before)
{
    return automix_share(P, sum, floor, D_before);
}

extern "C" void cmhip_automix_free(cmhip_automix_t *m) { stage_free(m); }

// device false (cmhip_test_automix_new_dry): the mirror and the checks, no device behind them
static int automix_init(cmhip_automix_t *m, bool device)
{
    const cmhip_automix_desc_t &d = m->d;
    const size_t S = d.streams;
    m->mirror.init(S, AUTOMIX_DEFAULT);
    if (!device)
        return COOLMIC_ERROR_NONE;
    if (m->open("automix_new", d.device, d.hip_stream, 2 * S * AGC_REC) ||
        m->array("automix_new", &m->d_table, S * m->nw * d.channels) || m->array("automix_new", &m->d_power, S * m->nw) ||
        m->array("automix_new", &m->d_gsum, S * m->nw) || m->array("automix_new", &m->d_nodes, S * ((size_t)m->nw + 1u)) ||
        m->array("automix_new", &m->d_state, S) || m->array("automix_new", &m->d_clips, S))
        return COOLMIC_ERROR_GENERIC;
    return COOLMIC_ERROR_NONE;
}

static cmhip_automix_t *automix_new(const cmhip_automix_desc_t *d, bool device)
{
    if (!d) {
        fail(COOLMIC_ERROR_FAULT, "automix_new: NULL argument");
        return nullptr;
    }
    if (!agc_geometry_ok(d->streams, d->channels, d->window_log2, d->max_frames)) {
        fail(COOLMIC_ERROR_INVAL, "automix_new: streams, channels (1..16), window_log2 (%u..%u) and max_frames (times "
             "channels below 2^31) out of range", AGC_W_MIN, AGC_W_MAX);
        return nullptr;
    }
    return stage_new<cmhip_automix>("automix_new", [&](cmhip_automix_t *m) {
        m->d = *d;
        m->nw = agc_table_windows(d->max_frames, d->window_log2);
        return automix_init(m, device);
    });
}

extern "C" cmhip_automix_t *cmhip_automix_new(const cmhip_automix_desc_t *d) { return automix_new(d, true); }

// test hook: an object with its mirror and every check but no device behind it, for the refusals and the mirror's
// answers on a machine without a GPU; a run that would launch is refused
extern "C" cmhip_automix_t *cmhip_test_automix_new_dry(const cmhip_automix_desc_t *d) { return automix_new(d, false); }

extern "C" void *cmhip_automix_hip_stream(cmhip_automix_t *m) { return m ? (void *)m->stream : nullptr; }

extern "C" int cmhip_automix_sync(cmhip_automix_t *m) { return stage_sync(m, "automix_sync"); }

extern "C" int cmhip_automix_set(cmhip_automix_t *m, long stream, const cmhip_automix_params_t *p)
{
    if (!p)
        return fail(COOLMIC_ERROR_FAULT, "automix_set: NULL argument");
    StreamRange sr;
    const int rc = stage_streams(m, "automix_set", stream, &sr);
    if (rc)
        return rc;
    const AutomixParams q = automix_from(p);
    if (!automix_params_ok(q))
        return fail(COOLMIC_ERROR_INVAL, "automix_set: %s", AUTOMIX_RANGES);
    for (size_t s = sr.lo; s < (size_t)sr.lo + sr.n; s++)
        m->mirror.par[s] = q;
    return COOLMIC_ERROR_NONE;
}

extern "C" int cmhip_automix_get(const cmhip_automix_t *m, unsigned stream, cmhip_automix_params_t *p)
{
    if (!m || !p)
        return fail(COOLMIC_ERROR_FAULT, "automix_get: NULL argument");
    if (stream >= m->d.streams)
        return fail(COOLMIC_ERROR_INVAL, "automix_get: stream %u out of range", stream);
    memcpy(p, &m->mirror.par[stream], sizeof(*p));
    return COOLMIC_ERROR_NONE;
}

// (the group id is checked against S here, so the device never indexes past gsum)
extern "C" int cmhip_automix_set_group(cmhip_automix_t *m, long stream, long group)
{
    if (!m)
        return fail(COOLMIC_ERROR_FAULT, "automix_set_group: NULL argument");
    if (stream < 0 || (unsigned long)stream >= m->d.streams)
        return fail(COOLMIC_ERROR_INVAL, "automix_set_group: stream %ld out of range", stream);
    if (group < -1 || (group >= 0 && (unsigned long)group >= m->d.streams))
        return fail(COOLMIC_ERROR_INVAL, "automix_set_group: group %ld out of range", group);
    m->mirror.set_group((size_t)stream, group < 0 ? AUTOMIX_NO_GROUP : (uint32_t)group);
    return COOLMIC_ERROR_NONE;
}

extern "C" int cmhip_automix_get_group(const cmhip_automix_t *m, unsigned stream, long *group)
{
    if (!m || !group)
        return fail(COOLMIC_ERROR_FAULT, "automix_get_group: NULL argument");
    if (stream >= m->d.streams)
        return fail(COOLMIC_ERROR_INVAL, "automix_get_group: stream %u out of range", stream);
    *group = m->mirror.group[stream] == AUTOMIX_NO_GROUP ? -1L : (long)m->mirror.group[stream];
    return COOLMIC_ERROR_NONE;
}

static int automix_run_on(cmhip_automix_t *m, const void *in, size_t in_stride, size_t frames,
                          const uint32_t *frames_per_stream, void *out, size_t out_stride, hipEvent_t *ev)
{
    if (!m)
        return fail(COOLMIC_ERROR_FAULT, "automix_run: NULL argument");
    const unsigned S = m->d.streams, C = m->d.channels;
    const StageRun r = {in, out, in_stride, out_stride, frames, m->d.max_frames, frames_per_stream, S, S, C, frames, C,
                        STAGE_APART};
    int rc = stage_run_refusal("automix_run", r);
    if (rc)
        return rc;
    // a group is on one clock: frame n of one member is frame n of every other.  The rule is judged on the mirror alone,
    // so it stands behind the run's own checks (which stage_run_begin repeats) and in front of "the object has no device"
    size_t sa = 0, sb = 0;
    if (frames_per_stream && !m->mirror.counts_agree([&](size_t s) { return frames_per_stream[s]; }, &sa, &sb))
        return fail(COOLMIC_ERROR_INVAL, "automix_run: stream %zu has %u frames, stream %zu of the same group (%u) has %u",
                    sa, frames_per_stream[sa], sb, m->mirror.group[sb], frames_per_stream[sb]);
    if (!stage_run_begin(m, "automix_run", r, &rc))
        return rc;
    if (plan_agc(S, C, m->d.window_log2, m->d.max_frames, (uint32_t)frames).err)
        return fail(COOLMIC_ERROR_INVAL, "automix_run: %u streams of %zu frames: the grid would reach 2^31 workgroups", S, frames);
    // nothing was touched so far; from here on the run happens
    // the run's records: the counts, and beside each the stream's position, parameters and group; behind them the same
    // with count 0 for the streams in no group
    uint32_t *block;
    HIP_TRY(m->counts.take(&block));
    const size_t words = (size_t)S * AGC_REC;
    for (unsigned s = 0; s < S; s++) {
        uint32_t *rec = block + (size_t)s * AGC_REC;
        m->mirror.record(s, stage_count(frames_per_stream, s, frames), rec);
        memcpy(rec + words, rec, AGC_REC * sizeof(uint32_t));
        if (m->mirror.group[s] == AUTOMIX_NO_GROUP)
            rec[words + AREC_COUNT] = 0;
    }
    HIP_TRY(m->counts.send(m->d_counts, 2 * words, m->stream));
    AutomixArgs a;
    memset(&a, 0, sizeof(a));
    a.tile.in = (const int16_t *)in;
    a.tile.out = (int16_t *)out;
    a.tile.rec = m->d_counts;
    a.tile.table = m->d_table;
    a.tile.nodes = m->d_nodes;
    a.tile.clips = m->d_clips;
    a.tile.in_stride = in_stride;
    a.tile.out_stride = out_stride;
    a.tile.streams = S;
    a.tile.channels = C;
    a.tile.w = m->d.window_log2;
    a.rec_energy = m->d_counts + words;
    a.power = m->d_power;
    a.gsum = m->d_gsum;
    a.state = m->d_state;
    rc = stage_launched("automix_run", launch_automix(a, m->d.max_frames, (uint32_t)frames, m->stream, ev));
    for (unsigned s = 0; s < S && !rc; s++)
        m->mirror.advance(s, stage_count(frames_per_stream, s, frames));
    return rc;
}

extern "C" int cmhip_automix_run(cmhip_automix_t *m, const void *in, size_t in_stride, size_t frames,
                                 const uint32_t *frames_per_stream, void *out, size_t out_stride)
{
    return automix_run_on(m, in, in_stride, frames, frames_per_stream, out, out_stride, nullptr);
}

// test hook: cmhip_automix_run with five of the caller's events (hipEvent_t [5]) recorded on the object's stream in
// front of, between and behind the four launches, so that tools/bench_automix.py can time each kernel by itself
extern "C" int cmhip_test_automix_run_events(cmhip_automix_t *m, const void *in, size_t in_stride, size_t frames,
                                             const uint32_t *frames_per_stream, void *out, size_t out_stride, void **events)
{
    if (!events)
        return fail(COOLMIC_ERROR_FAULT, "automix_run_events: NULL argument");
    return automix_run_on(m, in, in_stride, frames, frames_per_stream, out, out_stride, (hipEvent_t *)events);
}

extern "C" int cmhip_automix_reset(cmhip_automix_t *m, long stream)
{
    StreamRange sr;
    const int rc = stage_streams(m, "automix_reset", stream, &sr);
    if (rc)
        return rc;
    for (size_t s = sr.lo; s < (size_t)sr.lo + sr.n; s++)
        m->mirror.reset(s);                          // the next records say so, and the group starts afresh
    return COOLMIC_ERROR_NONE;
}

extern "C" int cmhip_automix_state(cmhip_automix_t *m, uint32_t *gain, uint64_t *power, uint32_t *share)
{
    if (!m)
        return fail(COOLMIC_ERROR_FAULT, "automix_state: NULL argument");
    return stage_guard("automix_state", [&] {
        const size_t S = m->d.streams;
        std::vector<AutomixState> st(S);
        if (stage_read(m, st.data(), m->d_state, S * sizeof(AutomixState), false))
            return COOLMIC_ERROR_GENERIC;
        for (size_t s = 0; s < S; s++) {
            const bool none = m->mirror.group[s] == AUTOMIX_NO_GROUP;
            const bool fresh = !m->opened || m->mirror.pos[s] == 0;  // before frame 0: what the device holds is stale
            const uint32_t first = none ? AUTOMIX_UNITY : m->mirror.par[s].initial;
            if (gain)
                gain[s] = none || fresh ? first : st[s].a_hi;
            if (power)
                power[s] = none || fresh ? 0u : st[s].power;
            if (share)
                share[s] = none || fresh ? first : st[s].pending;
        }
        return COOLMIC_ERROR_NONE;
    });
}
