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

#include <new>

struct cmhip_delay : StageBase {
    cmhip_delay_desc_t d;
    int16_t *d_ring;
    uint32_t cap;                      // frames of a stream's ring
    DelayMirror mirror;
    bool dry;                          // cmhip_test_delay_new_dry: the mirror and the checks, no device behind them
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

extern "C" void cmhip_delay_free(cmhip_delay_t *m)
{
    if (!m)
        return;
    if (!m->dry) {
        m->close();
        (void)hipFree(m->d_ring);
    }
    delete m;
}

static int delay_init(cmhip_delay_t *m)
{
    const cmhip_delay_desc_t &d = m->d;
    const size_t S = d.streams;
    try {
        m->mirror.init(S, m->cap);
    } catch (const std::bad_alloc &) {
        return fail(COOLMIC_ERROR_NOMEM, "delay_new: out of memory");
    }
    if (m->dry)
        return COOLMIC_ERROR_NONE;
    if (m->open(d.device, d.hip_stream, S * DELAY_REC))
        return COOLMIC_ERROR_GENERIC;
    const size_t bytes = S * (size_t)m->cap * d.channels * sizeof(int16_t);
    if (hipMalloc((void **)&m->d_ring, bytes) != hipSuccess) {
        (void)hipGetLastError();
        m->d_ring = nullptr;
        return fail(COOLMIC_ERROR_NOMEM, "delay_new: no device memory for %zu bytes of rings", bytes);
    }
    HIP_TRY(hipMemsetAsync(m->d_ring, 0, bytes, m->stream));
    return COOLMIC_ERROR_NONE;
}

static cmhip_delay_t *delay_new(const cmhip_delay_desc_t *d, bool dry)
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
    cmhip_delay_t *m = new (std::nothrow) cmhip_delay();
    if (!m) {
        fail(COOLMIC_ERROR_NOMEM, "delay_new: out of memory");
        return nullptr;
    }
    m->d = *d;
    m->dry = dry;
    m->cap = (uint32_t)delay_ring_frames(d->max_delay, d->max_frames);
    if (delay_init(m)) {
        cmhip_delay_free(m);
        return nullptr;
    }
    return m;
}

extern "C" cmhip_delay_t *cmhip_delay_new(const cmhip_delay_desc_t *d) { return delay_new(d, false); }

// test hook: an object with its mirror and every check but no device behind it, for the refusals and the mirror's
// answers on a machine without a GPU; a run that would launch is refused
extern "C" cmhip_delay_t *cmhip_test_delay_new_dry(const cmhip_delay_desc_t *d) { return delay_new(d, true); }

extern "C" size_t cmhip_delay_max_delay(const cmhip_delay_t *m) { return m ? m->d.max_delay : 0; }

extern "C" void *cmhip_delay_hip_stream(cmhip_delay_t *m) { return m ? (void *)m->stream : nullptr; }

extern "C" int cmhip_delay_sync(cmhip_delay_t *m) { return m && m->dry ? COOLMIC_ERROR_NONE : stage_sync(m, "delay_sync"); }

extern "C" int cmhip_delay_set(cmhip_delay_t *m, long stream, uint32_t delay)
{
    if (!m)
        return fail(COOLMIC_ERROR_FAULT, "delay_set: NULL argument");
    const StreamRange sr = stream_range(stream, m->d.streams);
    if (!sr.ok)
        return fail(COOLMIC_ERROR_INVAL, "delay_set: stream %ld out of range", stream);
    if (delay > m->d.max_delay)
        return fail(COOLMIC_ERROR_INVAL, "delay_set: %u frames above the object's %zu", delay, m->d.max_delay);
    for (size_t s = sr.lo; s < (size_t)sr.lo + sr.n; s++)
        m->mirror.set(s, delay);                     // a step ends whatever ramp runs
    return COOLMIC_ERROR_NONE;
}

extern "C" int cmhip_delay_ramp(cmhip_delay_t *m, long stream, uint32_t delay, uint32_t ramp_frames)
{
    if (!m)
        return fail(COOLMIC_ERROR_FAULT, "delay_ramp: NULL argument");
    const StreamRange sr = stream_range(stream, m->d.streams);
    if (!sr.ok)
        return fail(COOLMIC_ERROR_INVAL, "delay_ramp: stream %ld out of range", stream);
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
    const int refused = stage_run_refusal("delay_run", r);
    if (refused)
        return refused;
    // nothing was touched so far; from here on the run happens
    if (frames == 0)
        return COOLMIC_ERROR_NONE;
    if (m->dry)
        return fail(COOLMIC_ERROR_INVAL, "delay_run: the object has no device");
    HIP_TRY(hipSetDevice(m->d.device));
    if (plan_delay(S, C, (uint32_t)m->d.max_delay, (uint32_t)m->d.max_frames, (uint32_t)frames).err)
        return fail(COOLMIC_ERROR_INVAL, "delay_run: %u streams of %zu frames: the grid would reach 2^31 workgroups", S, frames);
    // the run's records: the counts, and beside each the stream's position, taps and place in its ramp
    uint32_t *block;
    HIP_TRY(m->counts.take(&block));
    for (unsigned s = 0; s < S; s++)
        m->mirror.record(s, frames_per_stream ? frames_per_stream[s] : (uint32_t)frames, block + (size_t)s * DELAY_REC);
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
    const hipError_t e = launch_delay(a, (uint32_t)m->d.max_delay, (uint32_t)m->d.max_frames, (uint32_t)frames, m->stream);
    if (e != hipSuccess)
        return fail(COOLMIC_ERROR_GENERIC, "delay_run: %s", hipGetErrorString(e));
    for (unsigned s = 0; s < S; s++)                 // the kernel wrote every stream's frames behind its position
        m->mirror.advance(s, frames_per_stream ? frames_per_stream[s] : (uint32_t)frames);
    return COOLMIC_ERROR_NONE;
}

extern "C" int cmhip_delay_reset(cmhip_delay_t *m, long stream)
{
    if (!m)
        return fail(COOLMIC_ERROR_FAULT, "delay_reset: NULL argument");
    const StreamRange sr = stream_range(stream, m->d.streams);
    if (!sr.ok)
        return fail(COOLMIC_ERROR_INVAL, "delay_reset: stream %ld out of range", stream);
    if (m->dry)
        return COOLMIC_ERROR_NONE;
    HIP_TRY(hipSetDevice(m->d.device));
    const size_t per = (size_t)m->cap * m->d.channels;
    HIP_TRY(hipMemsetAsync(m->d_ring + sr.lo * per, 0, sr.n * per * sizeof(int16_t), m->stream));
    return COOLMIC_ERROR_NONE;
}
