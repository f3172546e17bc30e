// cmhip_denoise.hip -- the noise suppressor on the host side (include/coolmic_hip.h, "noise suppressor"): the object
// beside the batch, its validation, the host's mirror of every stream's position, learning and parameters, the design of
// parameters from a law in dB and milliseconds, and the launch of k_denoise.hip's kernel.
//
// Device state of a suppressor: per row (stream, channel) the last N - 1 inputs in a history pair, the overlap-add tail,
// the gains, the profile and the learning sums; per stream the two counters.  Positions (back), the learn flag, the
// learning count and the parameters live in the host's mirror: the host sees every run's counts and every set, so a
// run's records travel to the device with the run, through the counts ring.  set, learn and reset therefore change the
// mirror alone and are ordered with the runs by the order of the calls; a profile travels through a pinned ring of its
// own and is copied in stream order.
#include "cmhip_engine.h"

#include <math.h>
#include <string.h>

static_assert(sizeof(cmhip_denoise_params_t) == sizeof(DenoiseParams) && sizeof(DenoiseParams) == 6,
              "cmhip_denoise_params_t is DenoiseParams");
static_assert(offsetof(cmhip_denoise_params_t, fall_shift) == offsetof(DenoiseParams, fall_shift),
              "cmhip_denoise_params_t is DenoiseParams");

struct cmhip_denoise : StageBase {
    cmhip_denoise_desc_t d;
    uint32_t bins;                     // N / 2 + 1
    HistoryPair hist;                  // [2][S][C][N]
    int32_t *d_table;                  // Wr[N/2], Wi[N/2], sw[N]
    int32_t *d_tail;                   // [S][C][N]
    uint32_t *d_gain;                  // [S][C][bins]
    unsigned long long *d_np, *d_acc;  // [S][C][bins]
    unsigned long long *d_clips, *d_sat;   // [S]
    CountsRing profiles;               // a profile on its way to d_np: 2 * bins dwords
    DenoiseMirror mirror;

    // (stage_free ends the object through this: the second ring goes once the stream is idle)
    void close()
    {
        if (opened) {
            (void)hipSetDevice(device);
            if (stream)
                (void)hipStreamSynchronize(stream);
            profiles.destroy();
        }
        StageBase::close();
    }
};

static const DenoiseParams DENOISE_DEFAULT = {32768, 16, 0, 0};

static DenoiseParams denoise_from(const cmhip_denoise_params_t *p)
{
    DenoiseParams q;
    memcpy(&q, p, sizeof(q));
    return q;
}

extern "C" int cmhip_denoise_check(unsigned int fft_log2, const cmhip_denoise_params_t *p)
{
    if (!denoise_log2_ok(fft_log2))
        return fail(COOLMIC_ERROR_INVAL, "denoise_check: fft_log2 %u outside %u..%u", fft_log2, SPEC_MIN_LOG2, SPEC_MAX_LOG2);
    if (p && !denoise_params_ok(denoise_from(p)))
        return fail(COOLMIC_ERROR_INVAL, "denoise_check: floor 0..32768 and shifts 0..8 are required");
    return COOLMIC_ERROR_NONE;
}

extern "C" int cmhip_denoise_window(unsigned int fft_log2, int16_t *win)
{
    if (!win)
        return fail(COOLMIC_ERROR_FAULT, "denoise_window: NULL argument");
    if (!denoise_log2_ok(fft_log2))
        return fail(COOLMIC_ERROR_INVAL, "denoise_window: fft_log2 %u outside %u..%u", fft_log2, SPEC_MIN_LOG2, SPEC_MAX_LOG2);
    denoise_window(fft_log2, win);
    return COOLMIC_ERROR_NONE;
}

extern "C" uint32_t cmhip_denoise_gain(uint64_t p, uint64_t np, unsigned int over, unsigned int floor)
{
    if (np > DENOISE_NP_MAX || over > 255u || floor > DENOISE_UNITY)
        return 0;
    return denoise_target(p, np, over, floor);
}

// the nearest shift for a time in milliseconds: 2^shift hops
static uint8_t denoise_shift(double ms, double rate, double hop)
{
    const double hops = ms * rate / 1000.0 / hop;
    if (!(hops > 1.0))
        return 0;
    const double v = rint(log2(hops));
    return (uint8_t)(v > (double)DENOISE_SHIFT_MAX ? (double)DENOISE_SHIFT_MAX : v);
}

extern "C" int cmhip_denoise_design(const cmhip_denoise_law_desc_t *law, cmhip_denoise_params_t *p)
{
    if (!law || !p)
        return fail(COOLMIC_ERROR_FAULT, "denoise_design: NULL argument");
    const double in[6] = {law->rate, law->fft_log2, law->reduction_db, law->over_db, law->attack_ms, law->release_ms};
    for (double v : in)
        if (!isfinite(v))
            return fail(COOLMIC_ERROR_INVAL, "denoise_design: a value is not finite");
    if (!(law->rate > 0.0) || law->fft_log2 != rint(law->fft_log2) || law->fft_log2 < (double)SPEC_MIN_LOG2 ||
        law->fft_log2 > (double)SPEC_MAX_LOG2)
        return fail(COOLMIC_ERROR_INVAL, "denoise_design: the rate must be positive and fft_log2 an integer in %u..%u",
                    SPEC_MIN_LOG2, SPEC_MAX_LOG2);
    if (law->reduction_db < 0.0 || law->attack_ms < 0.0 || law->release_ms < 0.0)
        return fail(COOLMIC_ERROR_INVAL, "denoise_design: a negative reduction or time");
    const double hop = ldexp(1.0, (int)law->fft_log2 - 1);
    DenoiseParams q;
    q.floor = (uint16_t)rint(32768.0 * pow(10.0, -law->reduction_db / 20.0));
    const double beta = rint(16.0 * pow(10.0, law->over_db / 10.0));
    q.over = (uint8_t)(beta > 255.0 ? 255.0 : beta);
    q.rise_shift = denoise_shift(law->attack_ms, law->rate, hop);
    q.fall_shift = denoise_shift(law->release_ms, law->rate, hop);
    memcpy(p, &q, sizeof(q));
    return COOLMIC_ERROR_NONE;
}

extern "C" void cmhip_denoise_free(cmhip_denoise_t *m) { stage_free(m); }

// device false (cmhip_test_denoise_new_dry): the mirror and the checks, no device behind them
static int denoise_init(cmhip_denoise_t *m, bool device)
{
    const cmhip_denoise_desc_t &d = m->d;
    const size_t S = d.streams, rows = S * d.channels, N = (size_t)1 << d.fft_log2;
    m->bins = (uint32_t)(N / 2 + 1);
    m->mirror.init(S, d.fft_log2, DENOISE_DEFAULT);
    if (!device)
        return COOLMIC_ERROR_NONE;
    if (m->open("denoise_new", d.device, d.hip_stream, S * DENOISE_REC) ||
        m->hist.init(*m, "denoise_new", S, d.channels * N) || m->alloc("denoise_new", &m->d_table, 2 * N) ||
        m->array("denoise_new", &m->d_tail, rows * N) ||
        m->array("denoise_new", &m->d_gain, rows * m->bins, DENOISE_UNITY) ||
        m->array("denoise_new", &m->d_np, rows * m->bins) || m->array("denoise_new", &m->d_acc, rows * m->bins) ||
        m->array("denoise_new", &m->d_clips, S) || m->array("denoise_new", &m->d_sat, S))
        return COOLMIC_ERROR_GENERIC;
    HIP_TRY(m->profiles.init(2 * (size_t)m->bins));
    std::vector<int32_t> table(2 * N);
    std::vector<int16_t> sw(N);
    spec_twiddles(d.fft_log2, table.data(), table.data() + N / 2);
    denoise_window(d.fft_log2, sw.data());
    for (size_t i = 0; i < N; i++)
        table[N + i] = sw[i];
    HIP_TRY(hipMemcpy(m->d_table, table.data(), 2 * N * sizeof(int32_t), hipMemcpyHostToDevice));
    return COOLMIC_ERROR_NONE;
}

static cmhip_denoise_t *denoise_new(const cmhip_denoise_desc_t *d, bool device)
{
    if (!d) {
        fail(COOLMIC_ERROR_FAULT, "denoise_new: NULL argument");
        return nullptr;
    }
    if (!denoise_geometry_ok(d->streams, d->channels, d->fft_log2, d->max_frames)) {
        fail(COOLMIC_ERROR_INVAL, "denoise_new: streams, channels (1..16), fft_log2 (%u..%u) and max_frames (times channels "
             "below 2^31) out of range", SPEC_MIN_LOG2, SPEC_MAX_LOG2);
        return nullptr;
    }
    cmhip_denoise_t *m = stage_new<cmhip_denoise>("denoise_new", [&](cmhip_denoise_t *o) {
        o->d = *d;
        return denoise_init(o, device);
    });
    return m;
}

extern "C" cmhip_denoise_t *cmhip_denoise_new(const cmhip_denoise_desc_t *d) { return denoise_new(d, true); }

// test hook: an object with its mirror and every check but no device behind it, for the refusals and the mirror's
// answers on a machine without a GPU; a run that would launch is refused
extern "C" cmhip_denoise_t *cmhip_test_denoise_new_dry(const cmhip_denoise_desc_t *d) { return denoise_new(d, false); }

extern "C" void *cmhip_denoise_hip_stream(cmhip_denoise_t *m) { return m ? (void *)m->stream : nullptr; }

extern "C" int cmhip_denoise_sync(cmhip_denoise_t *m) { return stage_sync(m, "denoise_sync"); }

extern "C" size_t cmhip_denoise_delay(const cmhip_denoise_t *m) { return m ? ((size_t)1 << m->d.fft_log2) - 1u : 0u; }

extern "C" int cmhip_denoise_set(cmhip_denoise_t *m, long stream, const cmhip_denoise_params_t *p)
{
    if (!p)
        return fail(COOLMIC_ERROR_FAULT, "denoise_set: NULL argument");
    StreamRange sr;
    const int rc = stage_streams(m, "denoise_set", stream, &sr);
    if (rc)
        return rc;
    const DenoiseParams q = denoise_from(p);
    if (!denoise_params_ok(q))
        return fail(COOLMIC_ERROR_INVAL, "denoise_set: floor 0..32768 and shifts 0..8 are required");
    for (size_t s = sr.lo; s < (size_t)sr.lo + sr.n; s++)
        m->mirror.par[s] = q;
    return COOLMIC_ERROR_NONE;
}

extern "C" int cmhip_denoise_get(const cmhip_denoise_t *m, unsigned stream, cmhip_denoise_params_t *p)
{
    if (!m || !p)
        return fail(COOLMIC_ERROR_FAULT, "denoise_get: NULL argument");
    if (stream >= m->d.streams)
        return fail(COOLMIC_ERROR_INVAL, "denoise_get: stream %u out of range", stream);
    memcpy(p, &m->mirror.par[stream], sizeof(*p));
    return COOLMIC_ERROR_NONE;
}

extern "C" int cmhip_denoise_learn(cmhip_denoise_t *m, long stream, int on)
{
    StreamRange sr;
    const int rc = stage_streams(m, "denoise_learn", stream, &sr);
    if (rc)
        return rc;
    for (size_t s = sr.lo; s < (size_t)sr.lo + sr.n; s++)
        m->mirror.set_learn(s, on != 0);
    return COOLMIC_ERROR_NONE;
}

extern "C" int cmhip_denoise_reset(cmhip_denoise_t *m, long stream)
{
    StreamRange sr;
    const int rc = stage_streams(m, "denoise_reset", stream, &sr);
    if (rc)
        return rc;
    for (size_t s = sr.lo; s < (size_t)sr.lo + sr.n; s++)
        m->mirror.reset(s);                          // the next record says so, and the kernel starts the rows afresh
    return COOLMIC_ERROR_NONE;
}

extern "C" int cmhip_denoise_set_profile(cmhip_denoise_t *m, unsigned stream, unsigned channel, const uint64_t *np)
{
    if (!m || !np)
        return fail(COOLMIC_ERROR_FAULT, "denoise_set_profile: NULL argument");
    if (stream >= m->d.streams || channel >= m->d.channels)
        return fail(COOLMIC_ERROR_INVAL, "denoise_set_profile: stream %u or channel %u out of range", stream, channel);
    for (uint32_t k = 0; k < m->bins; k++)
        if (np[k] > DENOISE_NP_MAX)
            return fail(COOLMIC_ERROR_INVAL, "denoise_set_profile: bin %u above 2^52", k);
    if (m->mirror.learn[stream])
        return fail(COOLMIC_ERROR_BUSY, "denoise_set_profile: stream %u learns", stream);
    if (!m->opened)
        return COOLMIC_ERROR_NONE;
    HIP_TRY(hipSetDevice(m->device));
    uint32_t *block;
    HIP_TRY(m->profiles.take(&block));
    memcpy(block, np, (size_t)m->bins * sizeof(uint64_t));
    const size_t row = (size_t)stream * m->d.channels + channel;
    HIP_TRY(m->profiles.send((uint32_t *)(m->d_np + row * m->bins), 2 * (size_t)m->bins, m->stream));
    return COOLMIC_ERROR_NONE;
}

extern "C" int cmhip_denoise_get_profile(cmhip_denoise_t *m, unsigned stream, unsigned channel, uint64_t *np, uint32_t *gain)
{
    if (!m)
        return fail(COOLMIC_ERROR_FAULT, "denoise_get_profile: NULL argument");
    if (stream >= m->d.streams || channel >= m->d.channels)
        return fail(COOLMIC_ERROR_INVAL, "denoise_get_profile: stream %u or channel %u out of range", stream, channel);
    const size_t row = (size_t)stream * m->d.channels + channel;
    if (stage_read(m, np, m->opened ? m->d_np + row * m->bins : nullptr, (size_t)m->bins * sizeof(uint64_t), false) ||
        stage_read(m, gain, m->opened ? m->d_gain + row * m->bins : nullptr, (size_t)m->bins * sizeof(uint32_t), false))
        return COOLMIC_ERROR_GENERIC;
    if (gain && (!m->opened || m->mirror.fresh[stream]))     // before frame 0: what the device holds is stale
        for (uint32_t k = 0; k < m->bins; k++)
            gain[k] = DENOISE_UNITY;
    return COOLMIC_ERROR_NONE;
}

extern "C" int cmhip_denoise_run(cmhip_denoise_t *m, const void *in, size_t in_stride, size_t frames,
                                 const uint32_t *frames_per_stream, void *out, size_t out_stride)
{
    if (!m)
        return fail(COOLMIC_ERROR_FAULT, "denoise_run: NULL argument");
    const unsigned S = m->d.streams, C = m->d.channels;
    const StageRun r = {in, out, in_stride, out_stride, frames, m->d.max_frames, frames_per_stream, S, S, C, frames, C,
                        STAGE_APART};
    int rc;
    if (!stage_run_begin(m, "denoise_run", r, &rc))
        return rc;
    // nothing was touched so far; from here on the run happens
    // the run's records: the counts, and beside each the stream's back, flags, learning count and parameters
    uint32_t *block;
    HIP_TRY(m->counts.take(&block));
    for (unsigned s = 0; s < S; s++)
        m->mirror.record(s, stage_count(frames_per_stream, s, frames), block + (size_t)s * DENOISE_REC);
    HIP_TRY(m->counts.send(m->d_counts, (size_t)S * DENOISE_REC, m->stream));
    DenoiseArgs a;
    memset(&a, 0, sizeof(a));
    a.in = (const int16_t *)in;
    a.out = (int16_t *)out;
    a.rec = m->d_counts;
    a.table = m->d_table;
    a.hist = m->hist.d;
    a.tail = m->d_tail;
    a.gain = m->d_gain;
    a.np = m->d_np;
    a.acc = m->d_acc;
    a.clips = m->d_clips;
    a.sat = m->d_sat;
    a.in_stride = in_stride;
    a.out_stride = out_stride;
    a.streams = S;
    a.channels = C;
    a.log2n = m->d.fft_log2;
    a.parity = m->hist.parity();
    rc = stage_launched("denoise_run", launch_denoise(a, m->stream));
    if (rc)
        return rc;
    m->hist.flip();
    for (unsigned s = 0; s < S; s++)
        m->mirror.advance(s, stage_count(frames_per_stream, s, frames));
    return COOLMIC_ERROR_NONE;
}

extern "C" int cmhip_denoise_state(cmhip_denoise_t *m, uint64_t *clips, uint64_t *sat, uint32_t *learned_blocks, int clear)
{
    if (!m)
        return fail(COOLMIC_ERROR_FAULT, "denoise_state: NULL argument");
    const size_t S = m->d.streams;
    if (stage_read(m, clips, m->d_clips, S * sizeof(uint64_t), clear != 0) ||
        stage_read(m, sat, m->d_sat, S * sizeof(uint64_t), clear != 0))
        return COOLMIC_ERROR_GENERIC;
    for (size_t s = 0; s < S && learned_blocks; s++)
        learned_blocks[s] = m->mirror.cnt[s];
    return COOLMIC_ERROR_NONE;
}
