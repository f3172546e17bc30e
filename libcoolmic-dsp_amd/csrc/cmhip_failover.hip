// cmhip_failover.hip -- the failover switch on the host side (include/coolmic_hip.h, "failover switch"): the object beside
// the batch, its validation, the host's mirror of every output's position, parameters and candidate list, the design of
// parameters from a law, and the launch of k_failover.hip's kernels.
//
// Device state of a switch: per output the open window's sums per candidate, the candidates' last levels, the packed
// counters and the plan word in force (FailoverState), and the changeover counter; per run the table of sums
// [O * 4][NW][C] and the plan words [O][NW + 1].  Positions, parameters and lists live in the host's mirror
// (csrc/failover_plan.h): the host sees every run's counts, every set and every new list, so a run's records travel to
// the device with the run, through the counts ring -- the O * 4 rows the energy pass reads, and behind them the O
// outputs' own.  A set, a set_sources or a reset therefore changes the mirror alone and is ordered with the runs by
// the order of the calls: an output whose record says position 0 starts afresh.
#include "cmhip_engine.h"

#include <math.h>
#include <string.h>

static_assert(sizeof(cmhip_failover_params_t) == sizeof(FailoverParams) && sizeof(FailoverParams) == 16,
              "cmhip_failover_params_t is FailoverParams");
static_assert(offsetof(cmhip_failover_params_t, force) == offsetof(FailoverParams, force),
              "cmhip_failover_params_t is FailoverParams");

struct cmhip_failover : StageBase {
    cmhip_failover_desc_t d;
    uint32_t nw;                       // windows per row in the tables
    unsigned long long *d_table;       // [O * 4][nw][C]
    uint32_t *d_plan;                  // [O][nw + 1]
    FailoverState *d_state;            // [O]
    unsigned long long *d_switches;    // [O]
    FailoverMirror mirror;
};

static const char FAILOVER_RANGES[] = "quiet 0..32767, fail_windows and return_windows 1..65535, fade_log2 from window_log2 "
                                      "to 16 and force -1..sources-1 are required";

static FailoverParams failover_from(const cmhip_failover_params_t *p)
{
    FailoverParams q;
    memcpy(&q, p, sizeof(q));
    return q;
}

static FailoverParams failover_default(uint32_t w)
{
    FailoverParams q;
    for (uint32_t i = 0; i < FO_SRC; i++)
        q.quiet[i] = (uint16_t)FO_QUIET_DEFAULT;
    q.fail_windows = q.return_windows = 1;
    q.fade_log2 = (uint16_t)w;
    q.force = -1;
    return q;
}

extern "C" int cmhip_failover_check(unsigned int window_log2, unsigned int n_sources, const cmhip_failover_params_t *p)
{
    if (!agc_window_ok(window_log2))
        return fail(COOLMIC_ERROR_INVAL, "failover_check: window_log2 %u outside %u..%u", window_log2, AGC_W_MIN, AGC_W_MAX);
    if (n_sources < 1 || n_sources > FO_SRC)
        return fail(COOLMIC_ERROR_INVAL, "failover_check: %u sources outside 1..%u", n_sources, FO_SRC);
    if (p && !failover_params_ok(failover_from(p), window_log2, n_sources))
        return fail(COOLMIC_ERROR_INVAL, "failover_check: %s", FAILOVER_RANGES);
    return COOLMIC_ERROR_NONE;
}

// rint(v) clamped to lo..hi (v not NaN)
static uint16_t failover_round(double v, double lo, double hi)
{
    v = rint(v);
    return (uint16_t)(v < lo ? lo : v > hi ? hi : v);
}

extern "C" int cmhip_failover_design(const cmhip_failover_law_desc_t *law, cmhip_failover_params_t *p)
{
    if (!law || !p)
        return fail(COOLMIC_ERROR_FAULT, "failover_design: NULL argument");
    const double in[9] = {law->rate, law->window_log2, law->quiet_db[0], law->quiet_db[1], law->quiet_db[2],
                          law->quiet_db[3], law->fail_s, law->return_s, law->fade_ms};
    for (double v : in)
        if (!isfinite(v))
            return fail(COOLMIC_ERROR_INVAL, "failover_design: a value is not finite");
    if (!(law->rate > 0.0) || law->window_log2 != rint(law->window_log2) || law->window_log2 < (double)AGC_W_MIN ||
        law->window_log2 > (double)AGC_W_MAX)
        return fail(COOLMIC_ERROR_INVAL, "failover_design: the rate must be positive and window_log2 an integer in %u..%u",
                    AGC_W_MIN, AGC_W_MAX);
    if (law->fail_s < 0.0 || law->return_s < 0.0)
        return fail(COOLMIC_ERROR_INVAL, "failover_design: a negative time");
    const double w = law->window_log2, W = ldexp(1.0, (int)w);
    FailoverParams q;
    for (uint32_t i = 0; i < FO_SRC; i++)
        q.quiet[i] = failover_round(32768.0 * pow(10.0, law->quiet_db[i] / 20.0), 0.0, 32767.0);
    q.fail_windows = failover_round(law->fail_s * law->rate / W, 1.0, 65535.0);
    q.return_windows = failover_round(law->return_s * law->rate / W, 1.0, 65535.0);
    q.fade_log2 = law->fade_ms > 0.0 ? failover_round(log2(law->fade_ms * law->rate / 1000.0), w, (double)FO_FADE_MAX)
                                     : (uint16_t)w;
    q.force = -1;
    memcpy(p, &q, sizeof(q));
    return COOLMIC_ERROR_NONE;
}

static uint64_t failover_packed(const uint32_t *run)
{
    uint64_t v = 0;
    for (uint32_t i = 0; i < FO_SRC; i++)
        v = failover_run_set(v, i, run[i] < FO_RUN_MAX ? run[i] : FO_RUN_MAX);
    return v;
}

extern "C" uint32_t cmhip_failover_step(unsigned int n_sources, const cmhip_failover_params_t *p, uint32_t cur,
                                        const uint32_t *live_run, const uint32_t *dead_run)
{
    if (!p || !live_run || !dead_run || n_sources < 1 || n_sources > FO_SRC || cur >= n_sources || p->force >= (int)n_sources)
        return cur;
    return failover_step(n_sources, failover_from(p), cur, failover_packed(live_run), failover_packed(dead_run));
}

// test hook: one window edge as k_failover_step takes it.  plan: the plan word before (from | to << 2 | phi << 4 |
// q << 16) -> the one behind; live_run and dead_run [4] are moved on by level [4] first; *switched: 1 where a
// changeover begins.
extern "C" uint32_t cmhip_test_failover_edge(uint32_t plan, unsigned int n_sources, const cmhip_failover_params_t *p,
                                             unsigned int window_log2, const uint32_t *level, uint32_t *live_run,
                                             uint32_t *dead_run, uint32_t *switched)
{
    if (!p || !level || !live_run || !dead_run || !switched || n_sources < 1 || n_sources > FO_SRC)
        return plan;
    const FailoverParams q = failover_from(p);
    uint64_t live = failover_packed(live_run), dead = failover_packed(dead_run);
    for (uint32_t i = 0; i < n_sources; i++)
        failover_count(level[i], q.quiet[i], i, live, dead);
    for (uint32_t i = 0; i < FO_SRC; i++) {
        live_run[i] = failover_run(live, i);
        dead_run[i] = failover_run(dead, i);
    }
    return failover_edge(plan, n_sources, q, window_log2, live, dead, switched);
}

// test hook: the plan word of window 0, and one sample of a fade
extern "C" uint32_t cmhip_test_failover_first(const cmhip_failover_params_t *p) { return p ? failover_first(failover_from(p)) : 0u; }

extern "C" int32_t cmhip_test_failover_fade(int16_t a, int16_t b, uint32_t d, uint32_t phi)
{
    return failover_fade(a, b, d, phi);
}

extern "C" void cmhip_failover_free(cmhip_failover_t *m) { stage_free(m); }

// device false (cmhip_test_failover_new_dry): the mirror and the checks, no device behind them
static int failover_init(cmhip_failover_t *m, bool device)
{
    const cmhip_failover_desc_t &d = m->d;
    const size_t O = d.outputs;
    m->mirror.init(O, d.streams, failover_default(d.window_log2));
    if (!device)
        return COOLMIC_ERROR_NONE;
    if (m->open("failover_new", d.device, d.hip_stream, O * (FO_SRC * AGC_REC + FO_REC)) ||
        m->array("failover_new", &m->d_table, O * FO_SRC * m->nw * d.channels) ||
        m->array("failover_new", &m->d_plan, O * ((size_t)m->nw + 1u)) || m->array("failover_new", &m->d_state, O) ||
        m->array("failover_new", &m->d_switches, O))
        return COOLMIC_ERROR_GENERIC;
    return COOLMIC_ERROR_NONE;
}

static cmhip_failover_t *failover_new(const cmhip_failover_desc_t *d, bool device)
{
    if (!d) {
        fail(COOLMIC_ERROR_FAULT, "failover_new: NULL argument");
        return nullptr;
    }
    if (!agc_geometry_ok(d->streams, d->channels, d->window_log2, d->max_frames) || d->outputs == 0 ||
        d->outputs >= (1u << 29)) {
        fail(COOLMIC_ERROR_INVAL, "failover_new: streams, outputs (below 2^29), channels (1..16), window_log2 (%u..%u) and "
             "max_frames (times channels below 2^31) out of range", AGC_W_MIN, AGC_W_MAX);
        return nullptr;
    }
    return stage_new<cmhip_failover>("failover_new", [&](cmhip_failover_t *m) {
        m->d = *d;
        m->nw = agc_table_windows(d->max_frames, d->window_log2);
        return failover_init(m, device);
    });
}

extern "C" cmhip_failover_t *cmhip_failover_new(const cmhip_failover_desc_t *d) { return failover_new(d, true); }

// test hook: an object with its mirror and every check but no device behind it, for the refusals and the mirror's
// answers on a machine without a GPU; a run that would launch is refused
extern "C" cmhip_failover_t *cmhip_test_failover_new_dry(const cmhip_failover_desc_t *d) { return failover_new(d, false); }

extern "C" void *cmhip_failover_hip_stream(cmhip_failover_t *m) { return m ? (void *)m->stream : nullptr; }

extern "C" int cmhip_failover_sync(cmhip_failover_t *m) { return stage_sync(m, "failover_sync"); }

// how set and reset begin: the outputs the call names, -1 for all of them
static int failover_outputs(const cmhip_failover_t *m, const char *who, long output, StreamRange *sr)
{
    if (!m)
        return fail(COOLMIC_ERROR_FAULT, "%s: NULL argument", who);
    *sr = stream_range(output, m->d.outputs);
    if (!sr->ok)
        return fail(COOLMIC_ERROR_INVAL, "%s: output %ld out of range", who, output);
    return COOLMIC_ERROR_NONE;
}

extern "C" int cmhip_failover_set(cmhip_failover_t *m, long output, const cmhip_failover_params_t *p)
{
    if (!p)
        return fail(COOLMIC_ERROR_FAULT, "failover_set: NULL argument");
    StreamRange sr;
    const int rc = failover_outputs(m, "failover_set", output, &sr);
    if (rc)
        return rc;
    const FailoverParams q = failover_from(p);
    for (size_t o = sr.lo; o < (size_t)sr.lo + sr.n; o++)
        if (!failover_params_ok(q, m->d.window_log2, m->mirror.K[o]))
            return fail(COOLMIC_ERROR_INVAL, "failover_set: output %zu (%u sources): %s", o, m->mirror.K[o], FAILOVER_RANGES);
    for (size_t o = sr.lo; o < (size_t)sr.lo + sr.n; o++)
        m->mirror.par[o] = q;
    return COOLMIC_ERROR_NONE;
}

extern "C" int cmhip_failover_get(const cmhip_failover_t *m, unsigned output, cmhip_failover_params_t *p)
{
    if (!m || !p)
        return fail(COOLMIC_ERROR_FAULT, "failover_get: NULL argument");
    if (output >= m->d.outputs)
        return fail(COOLMIC_ERROR_INVAL, "failover_get: output %u out of range", output);
    memcpy(p, &m->mirror.par[output], sizeof(*p));
    return COOLMIC_ERROR_NONE;
}

// (the slots are checked against S here, so the device never reads past the input array's slots)
extern "C" int cmhip_failover_set_sources(cmhip_failover_t *m, unsigned output, unsigned n, const uint32_t *streams)
{
    if (!m || !streams)
        return fail(COOLMIC_ERROR_FAULT, "failover_set_sources: NULL argument");
    if (output >= m->d.outputs)
        return fail(COOLMIC_ERROR_INVAL, "failover_set_sources: output %u out of range", output);
    if (!FailoverMirror::sources_ok(n, streams, m->d.streams))
        return fail(COOLMIC_ERROR_INVAL, "failover_set_sources: 1..%u different streams below %u are required", FO_SRC,
                    m->d.streams);
    m->mirror.set_sources(output, n, streams);
    return COOLMIC_ERROR_NONE;
}

extern "C" int cmhip_failover_get_sources(const cmhip_failover_t *m, unsigned output, unsigned *n, uint32_t *streams)
{
    if (!m || !n || !streams)
        return fail(COOLMIC_ERROR_FAULT, "failover_get_sources: NULL argument");
    if (output >= m->d.outputs)
        return fail(COOLMIC_ERROR_INVAL, "failover_get_sources: output %u out of range", output);
    *n = m->mirror.K[output];
    for (uint32_t i = 0; i < *n; i++)
        streams[i] = m->mirror.src[(size_t)output * FO_SRC + i];
    return COOLMIC_ERROR_NONE;
}

static int failover_run_on(cmhip_failover_t *m, const void *in, size_t in_stride, size_t frames,
                           const uint32_t *frames_per_output, void *out, size_t out_stride, hipEvent_t *ev)
{
    if (!m)
        return fail(COOLMIC_ERROR_FAULT, "failover_run: NULL argument");
    const unsigned S = m->d.streams, O = m->d.outputs, C = m->d.channels;
    // the counts are per OUTPUT slot: the run's checks see the two arrays, and the counts are held against `frames` here,
    // in the place cmhip_agc_run's refusals have them (behind frames > max_frames, in front of the strides)
    const StageRun r = {in, out, in_stride, out_stride, frames, m->d.max_frames, nullptr, S, O, C, frames, C, STAGE_APART};
    const StageRunError early = stage_run_check(r, nullptr);
    if ((early == STAGE_RUN_OK || early > STAGE_RUN_COUNT) && frames_per_output)
        for (unsigned o = 0; o < O; o++)
            if (frames_per_output[o] > frames)
                return fail(COOLMIC_ERROR_INVAL, "failover_run: frames_per_output[%u] above frames", o);
    int rc;
    if (!stage_run_begin(m, "failover_run", r, &rc))
        return rc;
    if (plan_agc(O * FO_SRC, C, m->d.window_log2, m->d.max_frames, (uint32_t)frames).err)
        return fail(COOLMIC_ERROR_INVAL, "failover_run: %u outputs of %zu frames: the grid would reach 2^31 workgroups", O, frames);
    // nothing was touched so far; from here on the run happens
    uint32_t *block;
    HIP_TRY(m->counts.take(&block));
    const size_t row_words = (size_t)O * FO_SRC * AGC_REC, words = row_words + (size_t)O * FO_REC;
    for (unsigned o = 0; o < O; o++) {
        const uint32_t count = stage_count(frames_per_output, o, frames);
        for (uint32_t i = 0; i < FO_SRC; i++)
            m->mirror.record_row(o, i, count, block + ((size_t)o * FO_SRC + i) * AGC_REC);
        m->mirror.record(o, count, block + row_words + (size_t)o * FO_REC);
    }
    HIP_TRY(m->counts.send(m->d_counts, words, m->stream));
    FailoverArgs a;
    memset(&a, 0, sizeof(a));
    a.energy.in = (const int16_t *)in;
    a.energy.rec = m->d_counts;
    a.energy.table = m->d_table;
    a.energy.in_stride = in_stride;
    a.energy.channels = C;
    a.energy.w = m->d.window_log2;
    a.out = (int16_t *)out;
    a.rec = m->d_counts + row_words;
    a.plan = m->d_plan;
    a.state = m->d_state;
    a.switches = m->d_switches;
    a.out_stride = out_stride;
    a.outputs = O;
    rc = stage_launched("failover_run", launch_failover(a, m->d.max_frames, (uint32_t)frames, m->stream, ev));
    for (unsigned o = 0; o < O && !rc; o++)
        m->mirror.advance(o, stage_count(frames_per_output, o, frames));
    return rc;
}

extern "C" int cmhip_failover_run(cmhip_failover_t *m, const void *in, size_t in_stride, size_t frames,
                                  const uint32_t *frames_per_output, void *out, size_t out_stride)
{
    return failover_run_on(m, in, in_stride, frames, frames_per_output, out, out_stride, nullptr);
}

// test hook: cmhip_failover_run with four of the caller's events (hipEvent_t [4]) recorded on the object's stream in
// front of, between and behind the three launches, so that tools/bench_failover.py can time each kernel by itself
extern "C" int cmhip_test_failover_run_events(cmhip_failover_t *m, const void *in, size_t in_stride, size_t frames,
                                              const uint32_t *frames_per_output, void *out, size_t out_stride, void **events)
{
    if (!events)
        return fail(COOLMIC_ERROR_FAULT, "failover_run_events: NULL argument");
    return failover_run_on(m, in, in_stride, frames, frames_per_output, out, out_stride, (hipEvent_t *)events);
}

extern "C" int cmhip_failover_reset(cmhip_failover_t *m, long output)
{
    StreamRange sr;
    const int rc = failover_outputs(m, "failover_reset", output, &sr);
    if (rc)
        return rc;
    for (size_t o = sr.lo; o < (size_t)sr.lo + sr.n; o++)
        m->mirror.reset(o);                          // the next record says so
    return COOLMIC_ERROR_NONE;
}

extern "C" int cmhip_failover_state(cmhip_failover_t *m, uint32_t *from, uint32_t *to, uint32_t *fade_window,
                                    uint64_t *switches, int clear, uint32_t *live_run, uint32_t *dead_run, uint32_t *level)
{
    if (!m)
        return fail(COOLMIC_ERROR_FAULT, "failover_state: NULL argument");
    return stage_guard("failover_state", [&] {
        const size_t O = m->d.outputs;
        std::vector<FailoverState> st(O);
        if (stage_read(m, st.data(), m->d_state, O * sizeof(FailoverState), false))
            return COOLMIC_ERROR_GENERIC;
        if ((switches || clear) && stage_read(m, switches, m->d_switches, O * sizeof(uint64_t), clear != 0))
            return COOLMIC_ERROR_GENERIC;
        for (size_t o = 0; o < O; o++) {
            const bool fresh = !m->opened || m->mirror.pos[o] == 0;  // before frame 0: what the device holds is stale
            const FailoverPlan pl = failover_plan_unpack(fresh ? failover_first(m->mirror.par[o]) : st[o].plan);
            if (from)
                from[o] = pl.from;
            if (to)
                to[o] = pl.to;
            if (fade_window)
                fade_window[o] = pl.q;
            for (uint32_t i = 0; i < FO_SRC; i++) {
                const bool none = fresh || i >= m->mirror.K[o];
                if (live_run)
                    live_run[o * FO_SRC + i] = none ? 0u : failover_run(st[o].live, i);
                if (dead_run)
                    dead_run[o * FO_SRC + i] = none ? 0u : failover_run(st[o].dead, i);
                if (level)
                    level[o * FO_SRC + i] = none ? 0u : st[o].level[i];
            }
        }
        return COOLMIC_ERROR_NONE;
    });
}
