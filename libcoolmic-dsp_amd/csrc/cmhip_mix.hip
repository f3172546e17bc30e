// cmhip_mix.hip -- channel mixing on the host side (include/coolmic_hip.h, "channel mixing"): the mixer object beside
// the batch, its validation, the launch of k_mix.hip's kernels, the presets and the matrix check.
//
// Device state of a mixer: the streams' matrices in the kernel's form (MixArgs::wk), uint32 [S][C_out][CP].  That is
// all: there is no history.  The host keeps a mirror of every matrix as the caller gave it (int16 [S][C_out][C_in]);
// cmhip_mix_get_matrix answers from it.  A new matrix reaches the device inside a kernel's arguments (k_mix_set), so
// it is ordered with the runs by the stream alone and no staging memory outlives the call.
//
// Matrix ramps (include/coolmic_hip.h, "matrix ramps"): the first cmhip_mix_ramp_matrix allocates a record per stream
// on the device (MixRampArgs::ramp) and the host's mirror of it (csrc/mix_ramp.h).  The host sees every run's counts,
// so the mirror advances as the device does and knows whether any stream ramps: only then does cmhip_mix_run launch
// k_mixramp.hip's kernels, and a mixer that never ramps launches what it always did.
#include "cmhip_engine.h"
#include "mix_ramp.h"

#include <stdlib.h>
#include <string.h>

#include <memory>

constexpr uint64_t MIX_MAX_SAMPLES = 1ull << 31;     // per slot and run: the kernels index a slot in 32 bits

struct cmhip_mix : StageBase {
    cmhip_mix_desc_t d;
    uint32_t *d_wk;
    std::vector<int16_t> w;            // the mirror: [S][C_out][C_in]
    uint32_t *d_ramp;                  // the streams' ramp records, allocated by the first ramp
    std::unique_ptr<MixRampMirror> ramp;       // ... and their mirror
};

static bool mix_channels_ok(unsigned ci, unsigned co) { return ci >= 1 && ci <= MAX_CH && co >= 1 && co <= MAX_CH; }

extern "C" int cmhip_mix_check(unsigned channels_in, unsigned channels_out, const int16_t *W)
{
    if (!mix_channels_ok(channels_in, channels_out))
        return fail(COOLMIC_ERROR_INVAL, "mix: %u -> %u channels: both must lie in 1..16", channels_in, channels_out);
    if (!W)
        return fail(COOLMIC_ERROR_FAULT, "mix: matrix is NULL");
    for (unsigned o = 0; o < channels_out; o++) {
        unsigned long sum = 0;
        for (unsigned c = 0; c < channels_in; c++)
            sum += (unsigned long)abs((int)W[(size_t)o * channels_in + c]);
        if (sum > 65535)
            return fail(COOLMIC_ERROR_INVAL, "mix: row %u has sum |w| = %lu above 65535", o, sum);
    }
    return COOLMIC_ERROR_NONE;
}

// the presets, as the header prints them
static const int16_t MIX_P_MONO_TO_STEREO[] = {16384, 16384};
static const int16_t MIX_P_STEREO_TO_MONO[] = {8192, 8192};
static const int16_t MIX_P_STEREO_TO_MS[] = {8192, 8192, 8192, -8192};
static const int16_t MIX_P_51_TO_STEREO[] = {16384, 0, 11585, 0, 11585, 0, 0, 16384, 11585, 0, 0, 11585};
static const int16_t MIX_P_51_TO_STEREO_NORM[] = {6786, 0, 4799, 0, 4799, 0, 0, 6786, 4799, 0, 0, 4799};

extern "C" int cmhip_mix_preset(unsigned preset, unsigned *channels_in, unsigned *channels_out, int16_t *W, size_t cap)
{
    unsigned ci, co;
    const int16_t *w;
    switch (preset) {
    case CMHIP_MIX_MONO_TO_STEREO: ci = 1; co = 2; w = MIX_P_MONO_TO_STEREO; break;
    case CMHIP_MIX_STEREO_TO_MONO: ci = 2; co = 1; w = MIX_P_STEREO_TO_MONO; break;
    case CMHIP_MIX_STEREO_TO_MS: ci = 2; co = 2; w = MIX_P_STEREO_TO_MS; break;
    case CMHIP_MIX_51_TO_STEREO: ci = 6; co = 2; w = MIX_P_51_TO_STEREO; break;
    case CMHIP_MIX_51_TO_STEREO_NORM: ci = 6; co = 2; w = MIX_P_51_TO_STEREO_NORM; break;
    default:
        return fail(COOLMIC_ERROR_INVAL, "mix_preset: no preset %u", preset);
    }
    if (W) {
        if (cap < (size_t)ci * co)
            return fail(COOLMIC_ERROR_INVAL, "mix_preset: room for %zu entries, the matrix has %u", cap, ci * co);
        memcpy(W, w, (size_t)ci * co * sizeof(int16_t));
    }
    if (channels_in)
        *channels_in = ci;
    if (channels_out)
        *channels_out = co;
    return COOLMIC_ERROR_NONE;
}

static int mix_init(cmhip_mix_t *m)
{
    const cmhip_mix_desc_t &d = m->d;
    const size_t S = d.streams, CI = d.channels_in, CO = d.channels_out, n = CO * ((CI + 1) / 2);
    if (m->open("mix_new", d.device, d.hip_stream, S) || m->array("mix_new", &m->d_wk, S * n))
        return COOLMIC_ERROR_GENERIC;
    // the matrix at creation: the leading channels kept, silence in extra outputs
    std::vector<int16_t> w0(CO * CI, 0);
    for (size_t o = 0; o < (CI < CO ? CI : CO); o++)
        w0[o * CI + o] = 16384;
    m->w.resize(S * CO * CI);
    for (size_t s = 0; s < S; s++)
        memcpy(&m->w[s * CO * CI], w0.data(), CO * CI * sizeof(int16_t));
    return stage_launched("mix_new", launch_mix_set(m->d_wk, 0, d.streams, d.channels_in, d.channels_out, w0.data(),
                                                    m->stream));
}

extern "C" void cmhip_mix_free(cmhip_mix_t *m) { stage_free(m); }

extern "C" cmhip_mix_t *cmhip_mix_new(const cmhip_mix_desc_t *d)
{
    if (!d) {
        fail(COOLMIC_ERROR_FAULT, "mix_new: NULL argument");
        return nullptr;
    }
    if (d->streams == 0 || !mix_channels_ok(d->channels_in, d->channels_out) || d->max_frames == 0) {
        fail(COOLMIC_ERROR_INVAL, "mix_new: streams, channels_in, channels_out (1..16) and max_frames must be positive");
        return nullptr;
    }
    const unsigned cmax = d->channels_in > d->channels_out ? d->channels_in : d->channels_out;
    if (d->max_frames > MIX_MAX_SAMPLES / cmax) {
        fail(COOLMIC_ERROR_INVAL, "mix_new: max_frames %zu: a slot of a run would pass 2^31 samples", d->max_frames);
        return nullptr;
    }
    if ((uint64_t)d->streams * MAX_CH * (MAX_CH / 2) >= (1ull << 31)) {
        fail(COOLMIC_ERROR_INVAL, "mix_new: %u streams: the matrix table would pass 2^31 entries", d->streams);
        return nullptr;
    }
    return stage_new<cmhip_mix>("mix_new", [&](cmhip_mix_t *m) {
        m->d = *d;
        return mix_init(m);
    });
}

extern "C" int cmhip_mix_set_matrix(cmhip_mix_t *m, long stream, const int16_t *W)
{
    if (!W)
        return fail(COOLMIC_ERROR_FAULT, "mix_set_matrix: NULL argument");
    StreamRange sr;
    int rc = stage_streams(m, "mix_set_matrix", stream, &sr);
    if (rc)
        return rc;
    const unsigned CI = m->d.channels_in, CO = m->d.channels_out;
    rc = cmhip_mix_check(CI, CO, W);
    if (rc)
        return rc;
    HIP_TRY(hipSetDevice(m->d.device));
    const uint32_t lo = sr.lo, n = sr.n;
    rc = stage_launched("mix_set_matrix", launch_mix_set(m->d_wk, lo, n, CI, CO, W, m->stream));
    if (rc)
        return rc;
    if (m->ramp) {                     // a step ends whatever ramp runs
        rc = stage_launched("mix_set_matrix", launch_mixramp_cancel(m->d_ramp, lo, n, CI, CO, m->stream));
        if (rc)
            return rc;
        for (size_t s = lo; s < (size_t)lo + n; s++)
            m->ramp->cancel(s, W);
    }
    for (size_t s = lo; s < (size_t)lo + n; s++)
        memcpy(&m->w[s * CO * CI], W, (size_t)CO * CI * sizeof(int16_t));
    return COOLMIC_ERROR_NONE;
}

// the ramp records and their mirror, on first use: every stream at rest (R = 0) on its matrix
static int mix_ramp_alloc(cmhip_mix_t *m)
{
    return stage_guard("mix_ramp_matrix", [&] {
        const size_t S = m->d.streams, n = (size_t)m->d.channels_out * m->d.channels_in;
        auto mirror = std::make_unique<MixRampMirror>();
        mirror->init(S, n, m->w.data());
        const int rc = m->array("mix_ramp_matrix", &m->d_ramp, S * mixramp_record_dwords(m->d.channels_in, m->d.channels_out));
        if (!rc)
            m->ramp = std::move(mirror);
        return rc;
    });
}

extern "C" int cmhip_mix_ramp_matrix(cmhip_mix_t *m, long stream, const int16_t *W, uint32_t ramp_frames)
{
    if (!W)
        return fail(COOLMIC_ERROR_FAULT, "mix_ramp_matrix: NULL argument");
    StreamRange sr;
    int rc = stage_streams(m, "mix_ramp_matrix", stream, &sr);
    if (rc)
        return rc;
    if (ramp_frames > MIX_RAMP_MAX)
        return fail(COOLMIC_ERROR_INVAL, "mix_ramp_matrix: %u frames above %u", ramp_frames, MIX_RAMP_MAX);
    if (ramp_frames < 2)
        return cmhip_mix_set_matrix(m, stream, W);
    const unsigned CI = m->d.channels_in, CO = m->d.channels_out;
    rc = cmhip_mix_check(CI, CO, W);
    if (rc)
        return rc;
    HIP_TRY(hipSetDevice(m->d.device));
    if (!m->ramp && (rc = mix_ramp_alloc(m)) != 0)
        return rc;
    const uint32_t lo = sr.lo, n = sr.n;
    rc = stage_launched("mix_ramp_matrix", launch_mixramp_start(m->d_ramp, m->d_wk, lo, n, CI, CO, W, ramp_frames, m->stream));
    if (rc)
        return rc;
    for (size_t s = lo; s < (size_t)lo + n; s++) {
        m->ramp->start(s, W, ramp_frames);
        memcpy(&m->w[s * CO * CI], W, (size_t)CO * CI * sizeof(int16_t));
    }
    return COOLMIC_ERROR_NONE;
}

extern "C" int cmhip_mix_ramp_state(const cmhip_mix_t *m, unsigned stream, uint32_t *done, uint32_t *ramp_frames,
                                    int16_t *W_now)
{
    if (!m || !done || !ramp_frames)
        return fail(COOLMIC_ERROR_FAULT, "mix_ramp_state: NULL argument");
    if (stream >= m->d.streams)
        return fail(COOLMIC_ERROR_INVAL, "mix_ramp_state: stream %u out of range", stream);
    const size_t n = (size_t)m->d.channels_out * m->d.channels_in;
    if (m->ramp && m->ramp->ramping(stream)) {
        *done = m->ramp->done[stream];
        *ramp_frames = m->ramp->R[stream];
        if (W_now)
            m->ramp->now(stream, W_now);
    } else {
        *done = *ramp_frames = 0;
        if (W_now)
            memcpy(W_now, &m->w[stream * n], n * sizeof(int16_t));
    }
    return COOLMIC_ERROR_NONE;
}

extern "C" uint32_t cmhip_mix_ramp_position(uint32_t n, uint32_t ramp_frames) { return mix_ramp_position(n, ramp_frames); }

extern "C" int16_t cmhip_mix_ramp_weight(int16_t w0, int16_t w1, uint32_t p) { return mix_ramp_weight(w0, w1, p); }

extern "C" int cmhip_mix_get_matrix(const cmhip_mix_t *m, unsigned stream, int16_t *W)
{
    if (!m || !W)
        return fail(COOLMIC_ERROR_FAULT, "mix_get_matrix: NULL argument");
    if (stream >= m->d.streams)
        return fail(COOLMIC_ERROR_INVAL, "mix_get_matrix: stream %u out of range", stream);
    const size_t n = (size_t)m->d.channels_out * m->d.channels_in;
    memcpy(W, &m->w[stream * n], n * sizeof(int16_t));
    return COOLMIC_ERROR_NONE;
}

extern "C" void *cmhip_mix_hip_stream(cmhip_mix_t *m) { return m ? (void *)m->stream : nullptr; }

extern "C" int cmhip_mix_sync(cmhip_mix_t *m) { return stage_sync(m, "mix_sync"); }

extern "C" int cmhip_mix_run(cmhip_mix_t *m, const void *in, size_t in_stride, size_t frames,
                             const uint32_t *frames_per_stream, void *out, size_t out_stride)
{
    if (!m)
        return fail(COOLMIC_ERROR_FAULT, "mix_run: NULL argument");
    const unsigned S = m->d.streams, CI = m->d.channels_in, CO = m->d.channels_out;
    // (the two arrays may not share a byte: a narrower output written over the input would race between tiles)
    const StageRun r = {in, out, in_stride, out_stride, frames, m->d.max_frames, frames_per_stream, S, S, CI, frames, CO,
                        STAGE_APART};
    int rc;
    if (!stage_run_begin(m, "mix_run", r, &rc))
        return rc;
    MixArgs a;
    memset(&a, 0, sizeof(a));
    a.in = (const int16_t *)in;
    a.out = (int16_t *)out;
    a.wk = m->d_wk;
    a.in_stride = in_stride;
    a.out_stride = out_stride;
    a.frames = (uint32_t)frames;
    a.streams = S;
    a.channels_in = CI;
    a.channels_out = CO;
    if (plan_mix(a).err != hipSuccess)
        return fail(COOLMIC_ERROR_INVAL, "mix_run: %u streams of %zu frames: the grid would reach 2^31 workgroups", S,
                    frames);
    // nothing was touched so far; from here on the run happens
    HIP_TRY(m->send_counts(frames_per_stream, S, &a.nframes));
    if (!m->ramp || !m->ramp->any())                 // nobody ramps: the plain kernels, as ever
        return stage_launched("mix_run", launch_mix(a, m->stream));
    // somebody ramps: the ramp kernels, then every stream's position moves on by its count, there and here
    MixRampArgs ra;
    ra.m = a;
    ra.ramp = m->d_ramp;
    hipError_t e = launch_mixramp(ra, m->stream);
    if (e == hipSuccess)
        e = launch_mixramp_advance(m->d_ramp, a.nframes, a.frames, S, CI, CO, m->stream);
    rc = stage_launched("mix_run", e);
    for (unsigned s = 0; s < S && !rc; s++)
        m->ramp->advance(s, stage_count(frames_per_stream, s, frames));
    return rc;
}
