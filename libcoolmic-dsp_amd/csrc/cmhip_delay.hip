// cmhip_delay.hip -- the delay stage on the host side (include/coolmic_hip.h, "delay"): the object beside the batch, its
// validation, the host's mirror of every stream's position, delay and ramp, and the launch of k_delay.hip's kernels.
//
// Device state of a delay: the streams' rings, int16 [S][cap * C] (csrc/delay_plan.h), and nothing else.  Positions,
// delays and ramps live in the host's mirror: the host sees every run's counts, so a run's records -- count, position,
// both taps and the ramp's place per stream -- travel to the device with the run, through the counts ring.  A set or a
// ramp therefore changes the mirror alone and is ordered with the runs by the order of the calls; cmhip_delay_get
// answers from the mirror.
#include "cmhip_engine.h"

#include <math.h>
#include <string.h>

struct cmhip_delay : StageBase {
    cmhip_delay_desc_t d;
    int16_t *d_ring;
    uint32_t cap;                      // frames of a stream's ring
    DelayMirror mirror;
};

extern "C" uint32_t cmhip_delay_ms(unsigned rate, double ms)
{
    const double f = rint((double)rate * ms / 1000.0);
    return f >= 0.0 && f <= 4294967295.0 ? (uint32_t)f : 0u;         // (a NaN fails both comparisons)
}

extern "C" int16_t cmhip_delay_crossfade(int16_t a, int16_t b, uint32_t p)
{
    if (p > 32768u)
        p = 32768u;
    const int32_t N = (int32_t)a * (int32_t)(32768u - p) + (int32_t)b * (int32_t)p;
    return (int16_t)((N + 16384) >> 15);
}

extern "C" void cmhip_delay_free(cmhip_delay_t *m) { stage_free(m); }

// device false (cmhip_test_delay_new_dry): the mirror and the checks, no device behind them
static int delay_init(cmhip_delay_t *m, bool device)
{
    const cmhip_delay_desc_t &d = m->d;
    const size_t S = d.streams;
    m->mirror.init(S, m->cap);
    if (!device)
        return COOLMIC_ERROR_NONE;
    if (m->open("delay_new", d.device, d.hip_stream, S * DELAY_REC) ||
        m->array("delay_new", &m->d_ring, S * (size_t)m->cap * d.channels))
        return COOLMIC_ERROR_GENERIC;
    return COOLMIC_ERROR_NONE;
}

static cmhip_delay_t *delay_new(const cmhip_delay_desc_t *d, bool device)
{
    if (!d) {
        fail(COOLMIC_ERROR_FAULT, "delay_new: NULL argument");
        return nullptr;
    }
    if (d->streams == 0 || d->channels == 0 || d->channels > MAX_CH || d->max_frames == 0) {
        fail(COOLMIC_ERROR_INVAL, "delay_new: streams, channels (1..16) and max_frames must be positive");
        return nullptr;
    }
    if (!delay_geometry_ok(d->streams, d->channels, d->max_delay, d->max_frames)) {
        fail(COOLMIC_ERROR_INVAL, "delay_new: max_delay %zu + max_frames %zu: a ring would reach 2^31 samples", d->max_delay,
             d->max_frames);
        return nullptr;
    }
    return stage_new<cmhip_delay>("delay_new", [&](cmhip_delay_t *m) {
        m->d = *d;
        m->cap = (uint32_t)delay_ring_frames(d->max_delay, d->max_frames);
        return delay_init(m, device);
    });
}

extern "C" cmhip_delay_t *cmhip_delay_new(const cmhip_delay_desc_t *d) { return delay_new(d, true); }

// test hook: an object with its mirror and every check but no device behind it, for the refusals and the mirror's
// answers on a machine without a GPU; a run that would launch is refused
extern "C" cmhip_delay_t *cmhip_test_delay_new_dry(const cmhip_delay_desc_t *d) { return delay_new(d, false); }

extern "C" size_t cmhip_delay_max_delay(const cmhip_delay_t *m) { return m ? m->d.max_delay : 0; }

extern "C" void *cmhip_delay_hip_stream(cmhip_delay_t *m) { return m ? (void *)m->stream : nullptr; }

extern "C" int cmhip_delay_sync(cmhip_delay_t *m) { return stage_sync(m, "delay_sync"); }

extern "C" int cmhip_delay_set(cmhip_delay_t *m, long stream, uint32_t delay)
{
    StreamRange sr;
    const int rc = stage_streams(m, "delay_set", stream, &sr);
    if (rc)
        return rc;
    if (delay > m->d.max_delay)
        return fail(COOLMIC_ERROR_INVAL, "delay_set: %u frames above the object's %zu", delay, m->d.max_delay);
    for (size_t s = sr.lo; s < (size_t)sr.lo + sr.n; s++)
        m->mirror.set(s, delay);                     // a step ends whatever ramp runs
    return COOLMIC_ERROR_NONE;
}

extern "C" int cmhip_delay_ramp(cmhip_delay_t *m, long stream, uint32_t delay, uint32_t ramp_frames)
{
    StreamRange sr;
    const int rc = stage_streams(m, "delay_ramp", stream, &sr);
    if (rc)
        return rc;
    if (delay > m->d.max_delay)
        return fail(COOLMIC_ERROR_INVAL, "delay_ramp: %u frames above the object's %zu", delay, m->d.max_delay);
    if (ramp_frames > DELAY_RAMP_MAX)
        return fail(COOLMIC_ERROR_INVAL, "delay_ramp: %u frames above %u", ramp_frames, DELAY_RAMP_MAX);
    if (ramp_frames < 2)
        return cmhip_delay_set(m, stream, delay);
    for (size_t s = sr.lo; s < (size_t)sr.lo + sr.n; s++)
        if (m->mirror.ramping(s))
            return fail(COOLMIC_ERROR_BUSY, "delay_ramp: stream %zu is %u frames into a ramp of %u", s, m->mirror.done[s],
                        m->mirror.R[s]);
    for (size_t s = sr.lo; s < (size_t)sr.lo + sr.n; s++)
        m->mirror.ramp(s, delay, ramp_frames);
    return COOLMIC_ERROR_NONE;
}

extern "C" int cmhip_delay_get(const cmhip_delay_t *m, unsigned stream, uint32_t *delay, uint32_t *from, uint32_t *done,
                               uint32_t *ramp_frames)
{
    if (!m || !delay)
        return fail(COOLMIC_ERROR_FAULT, "delay_get: NULL argument");
    if (stream >= m->d.streams)
        return fail(COOLMIC_ERROR_INVAL, "delay_get: stream %u out of range", stream);
    const DelayMirror &r = m->mirror;
    const bool ramping = r.ramping(stream);
    *delay = r.d1[stream];
    if (from)
        *from = ramping ? r.d0[stream] : r.d1[stream];
    if (done)
        *done = ramping ? r.done[stream] : 0u;
    if (ramp_frames)
        *ramp_frames = ramping ? r.R[stream] : 0u;
    return COOLMIC_ERROR_NONE;
}

extern "C" int cmhip_delay_run(cmhip_delay_t *m, const void *in, size_t in_stride, size_t frames,
                               const uint32_t *frames_per_stream, void *out, size_t out_stride)
{
    if (!m)
        return fail(COOLMIC_ERROR_FAULT, "delay_run: NULL argument");
    const unsigned S = m->d.streams, C = m->d.channels;
    const StageRun r = {in, out, in_stride, out_stride, frames, m->d.max_frames, frames_per_stream, S, S, C, frames, C,
                        STAGE_APART};
    int rc;
    if (!stage_run_begin(m, "delay_run", r, &rc))
        return rc;
    if (plan_delay(S, C, (uint32_t)m->d.max_delay, (uint32_t)m->d.max_frames, (uint32_t)frames).err)
        return fail(COOLMIC_ERROR_INVAL, "delay_run: %u streams of %zu frames: the grid would reach 2^31 workgroups", S, frames);
    // nothing was touched so far; from here on the run happens
    // the run's records: the counts, and beside each the stream's position, taps and place in its ramp
    uint32_t *block;
    HIP_TRY(m->counts.take(&block));
    for (unsigned s = 0; s < S; s++)
        m->mirror.record(s, stage_count(frames_per_stream, s, frames), block + (size_t)s * DELAY_REC);
    HIP_TRY(m->counts.send(m->d_counts, (size_t)S * DELAY_REC, m->stream));
    DelayArgs a;
    memset(&a, 0, sizeof(a));
    a.in = (const int16_t *)in;
    a.out = (int16_t *)out;
    a.ring = m->d_ring;
    a.rec = m->d_counts;
    a.in_stride = in_stride;
    a.out_stride = out_stride;
    a.ring_samples = m->cap * C;
    a.streams = S;
    a.channels = C;
    rc = stage_launched("delay_run", launch_delay(a, (uint32_t)m->d.max_delay, (uint32_t)m->d.max_frames, (uint32_t)frames,
                                                  m->stream));
    for (unsigned s = 0; s < S && !rc; s++)          // the kernel wrote every stream's frames behind its position
        m->mirror.advance(s, stage_count(frames_per_stream, s, frames));
    return rc;
}

extern "C" int cmhip_delay_reset(cmhip_delay_t *m, long stream)
{
    StreamRange sr;
    const int rc = stage_streams(m, "delay_reset", stream, &sr);
    if (rc || !m->opened)
        return rc;
    HIP_TRY(hipSetDevice(m->d.device));
    const size_t per = (size_t)m->cap * m->d.channels;
    HIP_TRY(hipMemsetAsync(m->d_ring + sr.lo * per, 0, sr.n * per * sizeof(int16_t), m->stream));
    return COOLMIC_ERROR_NONE;
}
