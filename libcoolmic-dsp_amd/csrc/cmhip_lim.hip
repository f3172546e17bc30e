// cmhip_lim.hip -- the peak limiter on the host side (include/coolmic_hip.h, "peak limiter"): the limiter object beside
// the batch, its validation, the launch of k_lim.hip's kernels (the sample detector) or k_limtp.hip's (the true-peak
// detector, fixed at creation), or k_limrel.hip's for either detector where the object has a release stage
// (release_log2 >= 1, fixed at creation), parameters, reset and the gain-reduction meter.
//
// Device state of a limiter: one parameter word per stream (threshold | drive << 16), the streams' history, int16
// [2][S][halo * C] raw input frames, two slots selected by a parity the host flips per run (the mechanism of
// cmhip_src.hip's d_hist), and the meter, uint32 [S].  The host keeps a mirror of the parameters; cmhip_lim_get answers
// from it.  New parameters reach the device inside a kernel's arguments (k_lim_set), so they are ordered with the runs
// by the stream alone and no staging memory outlives the call.
#include "cmhip_engine.h"

#include <math.h>
#include <string.h>

#include <new>

constexpr uint64_t LIM_MAX_SAMPLES = 1ull << 31;     // per slot and run: the kernels index a slot in 32 bits

struct cmhip_lim : StageBase {
    cmhip_lim_desc_t d;
    LimGeom g;                         // of the detector and the release: D, HIST and halo differ
    unsigned detector;
    unsigned rho;                      // release_log2; 0: no release stage
    uint32_t *d_par;
    uint32_t *d_gmin;
    int16_t *d_hist;
    unsigned parity;
    std::vector<uint32_t> par;         // the mirror: threshold | drive << 16
};

static size_t lim_slot(const cmhip_lim_t *m) { return (size_t)m->g.halo * m->d.channels; }     // samples per stream

extern "C" int cmhip_lim_check(unsigned lookahead_log2, unsigned hold, unsigned threshold, unsigned drive)
{
    if (!lim_geom(lookahead_log2, hold, nullptr))
        return fail(COOLMIC_ERROR_INVAL, "lim: lookahead_log2 %u, hold %u: 3..9, and 2^lookahead_log2 + hold <= 2048",
                    lookahead_log2, hold);
    if (!lim_params_ok(threshold, drive))
        return fail(COOLMIC_ERROR_INVAL, "lim: threshold %u, drive %u: 1..32767 and 1..65535", threshold, drive);
    return COOLMIC_ERROR_NONE;
}

extern "C" int cmhip_lim_check_detector(unsigned detector, unsigned lookahead_log2, unsigned hold, unsigned threshold,
                                        unsigned drive)
{
    if (detector == CMHIP_LIM_DETECT_SAMPLE)
        return cmhip_lim_check(lookahead_log2, hold, threshold, drive);
    if (detector != CMHIP_LIM_DETECT_TRUE_PEAK)
        return fail(COOLMIC_ERROR_INVAL, "lim: detector %u: 0 (sample) or 1 (true peak)", detector);
    if (!lim_geom_tp(lookahead_log2, hold, nullptr))
        return fail(COOLMIC_ERROR_INVAL, "lim: true-peak detector: lookahead_log2 %u, hold %u: 3..9, hold >= 1, and "
                    "2 * 2^lookahead_log2 + hold <= 2549", lookahead_log2, hold);
    if (!lim_params_ok(threshold, drive))
        return fail(COOLMIC_ERROR_INVAL, "lim: threshold %u, drive %u: 1..32767 and 1..65535", threshold, drive);
    return COOLMIC_ERROR_NONE;
}

extern "C" int cmhip_lim_check_release(unsigned detector, unsigned lookahead_log2, unsigned hold, unsigned release_log2,
                                       unsigned threshold, unsigned drive)
{
    const int rc = cmhip_lim_check_detector(detector, lookahead_log2, hold, threshold, drive);
    if (rc)
        return rc;
    if (!lim_geom_rel(detector, lookahead_log2, hold, release_log2, nullptr))
        return fail(COOLMIC_ERROR_INVAL, "lim: release_log2 %u (lookahead_log2 %u, hold %u): 0..11, and HIST = 2 * "
                    "2^lookahead_log2 + hold - 2 + 2^release_log2 - 1 (+ 13 with the true-peak detector) <= 4096",
                    release_log2, lookahead_log2, hold);
    return COOLMIC_ERROR_NONE;
}

extern "C" unsigned cmhip_lim_threshold_dbtp(double dbtp)
{
    if (isnan(dbtp))
        return 0u;
    const double t = floor(32768.0 * pow(10.0, dbtp / 20.0));
    return t < 1.0 ? 1u : t > (double)LIM_T_MAX ? LIM_T_MAX : (unsigned)t;
}

static int lim_init(cmhip_lim_t *m)
{
    const cmhip_lim_desc_t &d = m->d;
    const size_t S = d.streams;
    if (m->open(d.device, d.hip_stream, S))
        return COOLMIC_ERROR_GENERIC;
    HIP_TRY(hipMalloc((void **)&m->d_par, S * sizeof(uint32_t)));
    HIP_TRY(hipMalloc((void **)&m->d_gmin, S * sizeof(uint32_t)));
    HIP_TRY(hipMalloc((void **)&m->d_hist, 2 * S * lim_slot(m) * sizeof(int16_t)));
    HIP_TRY(hipMemsetAsync(m->d_hist, 0, 2 * S * lim_slot(m) * sizeof(int16_t), m->stream));
    HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)m->d_gmin, (int)LIM_UNITY, S, m->stream));
    m->par.assign(S, LIM_T_MAX | 4096u << 16);       // at creation: no limiting below full scale, unity drive
    const hipError_t e = launch_lim_set(m->d_par, 0, d.streams, LIM_T_MAX, 4096u, m->stream);
    if (e != hipSuccess)
        return fail(COOLMIC_ERROR_GENERIC, "lim_new: %s", hipGetErrorString(e));
    return COOLMIC_ERROR_NONE;
}

extern "C" void cmhip_lim_free(cmhip_lim_t *m)
{
    if (!m)
        return;
    m->close();
    (void)hipFree(m->d_par);
    (void)hipFree(m->d_gmin);
    (void)hipFree(m->d_hist);
    delete m;
}

extern "C" cmhip_lim_t *cmhip_lim_new(const cmhip_lim_desc_t *d)
{
    return cmhip_lim_new_detector(d, CMHIP_LIM_DETECT_SAMPLE);
}

extern "C" cmhip_lim_t *cmhip_lim_new_detector(const cmhip_lim_desc_t *d, unsigned detector)
{
    return cmhip_lim_new_release(d, detector, 0);
}

extern "C" cmhip_lim_t *cmhip_lim_new_release(const cmhip_lim_desc_t *d, unsigned detector, unsigned release_log2)
{
    if (!d) {
        fail(COOLMIC_ERROR_FAULT, "lim_new: NULL argument");
        return nullptr;
    }
    if (detector > CMHIP_LIM_DETECT_TRUE_PEAK) {
        fail(COOLMIC_ERROR_INVAL, "lim_new: detector %u: 0 (sample) or 1 (true peak)", detector);
        return nullptr;
    }
    LimGeom g;
    if (detector == CMHIP_LIM_DETECT_TRUE_PEAK && lim_geom(d->lookahead_log2, d->hold, &g) &&
        !lim_geom_tp(g.a, g.H, nullptr)) {           // (a geometry the sample detector would take)
        fail(COOLMIC_ERROR_INVAL, "lim_new: the true-peak detector needs hold >= 1 and 2 * 2^lookahead_log2 + hold <= "
             "2549 (lookahead_log2 %u, hold %u)", d->lookahead_log2, d->hold);
        return nullptr;
    }
    if (d->streams == 0 || d->channels == 0 || d->channels > MAX_CH || d->max_frames == 0 ||
        !lim_geom_of(detector, d->lookahead_log2, d->hold, &g)) {
        fail(COOLMIC_ERROR_INVAL, "lim_new: streams, channels (1..16) and max_frames must be positive, lookahead_log2 "
             "in 3..9 and 2^lookahead_log2 + hold <= 2048");
        return nullptr;
    }
    if (!lim_geom_rel(detector, g.a, g.H, release_log2, &g)) {       // (release_log2 0 leaves g as it is)
        fail(COOLMIC_ERROR_INVAL, "lim_new: release_log2 %u (lookahead_log2 %u, hold %u): 0..11, and the history, 2 * "
             "2^lookahead_log2 + hold - 2 + 2^release_log2 - 1 frames (+ 13 with the true-peak detector), may not pass "
             "4096", release_log2, d->lookahead_log2, d->hold);
        return nullptr;
    }
    if (d->max_frames > LIM_MAX_SAMPLES / d->channels) {
        fail(COOLMIC_ERROR_INVAL, "lim_new: max_frames %zu: a slot of a run would pass 2^31 samples", d->max_frames);
        return nullptr;
    }
    if ((uint64_t)d->streams * g.halo * d->channels >= (1ull << 31)) {
        fail(COOLMIC_ERROR_INVAL, "lim_new: %u streams: the history would pass 2^31 samples", d->streams);
        return nullptr;
    }
    cmhip_lim_t *m = new (std::nothrow) cmhip_lim();
    if (!m) {
        fail(COOLMIC_ERROR_NOMEM, "lim_new: out of memory");
        return nullptr;
    }
    m->d = *d;
    m->g = g;
    m->detector = detector;
    m->rho = release_log2;
    if (lim_init(m)) {
        cmhip_lim_free(m);
        return nullptr;
    }
    return m;
}

extern "C" unsigned cmhip_lim_delay(const cmhip_lim_t *m) { return m ? m->g.D : 0u; }

extern "C" unsigned cmhip_lim_detector(const cmhip_lim_t *m) { return m ? m->detector : 0u; }

extern "C" unsigned cmhip_lim_release(const cmhip_lim_t *m) { return m ? m->rho : 0u; }

extern "C" int cmhip_lim_set(cmhip_lim_t *m, long stream, unsigned threshold, unsigned drive)
{
    if (!m)
        return fail(COOLMIC_ERROR_FAULT, "lim_set: limiter is NULL");
    const StreamRange sr = stream_range(stream, m->d.streams);
    if (!sr.ok)
        return fail(COOLMIC_ERROR_INVAL, "lim_set: stream %ld out of range", stream);
    const int rc = cmhip_lim_check_detector(m->detector, m->g.a, m->g.H, threshold, drive);
    if (rc)
        return rc;
    HIP_TRY(hipSetDevice(m->d.device));
    const hipError_t e = launch_lim_set(m->d_par, sr.lo, sr.n, threshold, drive, m->stream);
    if (e != hipSuccess)
        return fail(COOLMIC_ERROR_GENERIC, "lim_set: %s", hipGetErrorString(e));
    for (size_t s = sr.lo; s < (size_t)sr.lo + sr.n; s++)
        m->par[s] = threshold | drive << 16;
    return COOLMIC_ERROR_NONE;
}

extern "C" int cmhip_lim_get(const cmhip_lim_t *m, unsigned stream, unsigned *threshold, unsigned *drive)
{
    if (!m)
        return fail(COOLMIC_ERROR_FAULT, "lim_get: limiter is NULL");
    if (stream >= m->d.streams)
        return fail(COOLMIC_ERROR_INVAL, "lim_get: stream %u out of range", stream);
    if (threshold)
        *threshold = m->par[stream] & 0xffffu;
    if (drive)
        *drive = m->par[stream] >> 16;
    return COOLMIC_ERROR_NONE;
}

extern "C" void *cmhip_lim_hip_stream(cmhip_lim_t *m) { return m ? (void *)m->stream : nullptr; }

extern "C" int cmhip_lim_sync(cmhip_lim_t *m) { return stage_sync(m, "lim_sync"); }

extern "C" int cmhip_lim_reset(cmhip_lim_t *m, long stream)
{
    if (!m)
        return fail(COOLMIC_ERROR_FAULT, "lim_reset: limiter is NULL");
    const StreamRange sr = stream_range(stream, m->d.streams);
    if (!sr.ok)
        return fail(COOLMIC_ERROR_INVAL, "lim_reset: stream %ld out of range", stream);
    HIP_TRY(hipSetDevice(m->d.device));
    const size_t lo = sr.lo, n = sr.n, per = lim_slot(m);
    // (the slot the next run reads; the other one is rewritten by that run)
    HIP_TRY(hipMemsetAsync(m->d_hist + ((size_t)m->parity * m->d.streams + lo) * per, 0, n * per * sizeof(int16_t),
                           m->stream));
    HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)(m->d_gmin + lo), (int)LIM_UNITY, n, m->stream));
    return COOLMIC_ERROR_NONE;
}

extern "C" int cmhip_lim_min_gain(cmhip_lim_t *m, uint32_t *out, int reset)
{
    if (!m || !out)
        return fail(COOLMIC_ERROR_FAULT, "lim_min_gain: NULL argument");
    HIP_TRY(hipSetDevice(m->d.device));
    HIP_TRY(hipMemcpyAsync(out, m->d_gmin, m->d.streams * sizeof(uint32_t), hipMemcpyDeviceToHost, m->stream));
    HIP_TRY(hipStreamSynchronize(m->stream));
    if (reset)
        HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)m->d_gmin, (int)LIM_UNITY, m->d.streams, m->stream));
    return COOLMIC_ERROR_NONE;
}

extern "C" int cmhip_lim_run(cmhip_lim_t *m, const void *in, size_t in_stride, size_t frames,
                             const uint32_t *frames_per_stream, void *out, size_t out_stride)
{
    if (!m)
        return fail(COOLMIC_ERROR_FAULT, "lim_run: NULL argument");
    const unsigned S = m->d.streams, C = m->d.channels;
    // (the two arrays may not share a byte: a tile reads the frames in front of it again after its neighbour may have
    // written them)
    const StageRun r = {in, out, in_stride, out_stride, frames, m->d.max_frames, frames_per_stream, S, S, C, frames, C,
                        STAGE_APART};
    const int refused = stage_run_refusal("lim_run", r);
    if (refused)
        return refused;
    if (plan_limrel(m->detector, S, C, m->g.a, m->g.H, m->rho, (uint32_t)frames).err)
        return fail(COOLMIC_ERROR_INVAL, "lim_run: %u streams of %zu frames: the grid would reach 2^31 workgroups", S,
                    frames);
    // nothing was touched so far; from here on the run happens
    if (frames == 0)
        return COOLMIC_ERROR_NONE;
    HIP_TRY(hipSetDevice(m->d.device));
    LimArgs a;
    memset(&a, 0, sizeof(a));
    a.in = (const int16_t *)in;
    a.out = (int16_t *)out;
    a.nframes = frames_per_stream ? m->d_counts : nullptr;
    a.par = m->d_par;
    a.hist = m->d_hist;
    a.gmin = m->d_gmin;
    a.in_stride = in_stride;
    a.out_stride = out_stride;
    a.frames = (uint32_t)frames;
    a.streams = S;
    a.channels = C;
    a.parity = m->parity;
    a.a = m->g.a;
    a.W = m->g.W;
    if (frames_per_stream)
        HIP_TRY(m->counts.upload(m->d_counts, frames_per_stream, S, m->stream));
    const hipError_t e = launch_limrel(a, m->detector, m->rho, m->stream);
    if (e != hipSuccess)
        return fail(COOLMIC_ERROR_GENERIC, "lim_run: %s", hipGetErrorString(e));
    m->parity ^= 1u;                         // the kernel wrote the other slots
    return COOLMIC_ERROR_NONE;
}
