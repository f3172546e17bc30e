// cmhip_lim.hip -- the peak limiter on the host side (include/coolmic_hip.h, "peak limiter"): the limiter object beside
// the batch, its validation, the launch of k_lim.hip's kernels (the sample detector) or k_limtp.hip's (the true-peak
// detector, fixed at creation), or k_limrel.hip's for either detector where the object has a release stage
// (release_log2 >= 1, fixed at creation), parameters, reset and the gain-reduction meter.
//
// Device state of a limiter: one parameter word per stream (threshold | drive << 16), the streams' history, int16
// [2][S][halo * C] raw input frames, two slots selected by a parity the host flips per run (HistoryPair,
// csrc/cmhip_stage.h), and the meter, uint32 [S].  The host keeps a mirror of the parameters; cmhip_lim_get answers
// from it.  New parameters reach the device inside a kernel's arguments (k_lim_set), so they are ordered with the runs
// by the stream alone and no staging memory outlives the call.
#include "cmhip_engine.h"

#include <math.h>
#include <string.h>

constexpr uint64_t LIM_MAX_SAMPLES = 1ull << 31;     // per slot and run: the kernels index a slot in 32 bits

struct cmhip_lim : StageBase {
    cmhip_lim_desc_t d;
    LimGeom g;                         // of the detector and the release: D, HIST and halo differ
    unsigned detector;
    unsigned rho;                      // release_log2; 0: no release stage
    uint32_t *d_par;
    uint32_t *d_gmin;
    HistoryPair hist;                  // [2][S][halo * C]
    std::vector<uint32_t> par;         // the mirror: threshold | drive << 16
};

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
    if (m->open("lim_new", d.device, d.hip_stream, S) || m->array("lim_new", &m->d_par, S) ||
        m->array("lim_new", &m->d_gmin, S, LIM_UNITY) || m->hist.init(*m, "lim_new", S, (size_t)m->g.halo * d.channels))
        return COOLMIC_ERROR_GENERIC;
    m->par.assign(S, LIM_T_MAX | 4096u << 16);       // at creation: no limiting below full scale, unity drive
    return stage_launched("lim_new", launch_lim_set(m->d_par, 0, d.streams, LIM_T_MAX, 4096u, m->stream));
}

extern "C" void cmhip_lim_free(cmhip_lim_t *m) { stage_free(m); }

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
    return stage_new<cmhip_lim>("lim_new", [&](cmhip_lim_t *m) {
        m->d = *d;
        m->g = g;
        m->detector = detector;
        m->rho = release_log2;
        return lim_init(m);
    });
}

extern "C" unsigned cmhip_lim_delay(const cmhip_lim_t *m) { return m ? m->g.D : 0u; }

extern "C" unsigned cmhip_lim_detector(const cmhip_lim_t *m) { return m ? m->detector : 0u; }

extern "C" unsigned cmhip_lim_release(const cmhip_lim_t *m) { return m ? m->rho : 0u; }

extern "C" int cmhip_lim_set(cmhip_lim_t *m, long stream, unsigned threshold, unsigned drive)
{
    StreamRange sr;
    int rc = stage_streams(m, "lim_set", stream, &sr);
    if (!rc)
        rc = cmhip_lim_check_detector(m->detector, m->g.a, m->g.H, threshold, drive);
    if (rc)
        return rc;
    HIP_TRY(hipSetDevice(m->d.device));
    rc = stage_launched("lim_set", launch_lim_set(m->d_par, sr.lo, sr.n, threshold, drive, m->stream));
    if (rc)
        return rc;
    for (size_t s = sr.lo; s < (size_t)sr.lo + sr.n; s++)
        m->par[s] = threshold | drive << 16;
    return COOLMIC_ERROR_NONE;
}

extern "C" int cmhip_lim_get(const cmhip_lim_t *m, unsigned stream, unsigned *threshold, unsigned *drive)
{
    if (!m)
        return fail(COOLMIC_ERROR_FAULT, "lim_get: NULL argument");
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
    StreamRange sr;
    const int rc = stage_streams(m, "lim_reset", stream, &sr);
    if (rc)
        return rc;
    HIP_TRY(hipSetDevice(m->d.device));
    HIP_TRY(m->hist.reset(sr.lo, sr.n, m->stream));
    HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)(m->d_gmin + sr.lo), (int)LIM_UNITY, sr.n, m->stream));
    return COOLMIC_ERROR_NONE;
}

extern "C" int cmhip_lim_min_gain(cmhip_lim_t *m, uint32_t *out, int reset)
{
    if (!m || !out)
        return fail(COOLMIC_ERROR_FAULT, "lim_min_gain: NULL argument");
    return stage_read(m, out, m->d_gmin, m->d.streams * sizeof(uint32_t), reset != 0, LIM_UNITY);
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
    int rc;
    if (!stage_run_begin(m, "lim_run", r, &rc))
        return rc;
    if (plan_limrel(m->detector, S, C, m->g.a, m->g.H, m->rho, (uint32_t)frames).err)
        return fail(COOLMIC_ERROR_INVAL, "lim_run: %u streams of %zu frames: the grid would reach 2^31 workgroups", S,
                    frames);
    // nothing was touched so far; from here on the run happens
    LimArgs a;
    memset(&a, 0, sizeof(a));
    a.in = (const int16_t *)in;
    a.out = (int16_t *)out;
    a.par = m->d_par;
    a.hist = m->hist.d;
    a.gmin = m->d_gmin;
    a.in_stride = in_stride;
    a.out_stride = out_stride;
    a.frames = (uint32_t)frames;
    a.streams = S;
    a.channels = C;
    a.parity = m->hist.parity();
    a.a = m->g.a;
    a.W = m->g.W;
    HIP_TRY(m->send_counts(frames_per_stream, S, &a.nframes));
    rc = stage_launched("lim_run", launch_limrel(a, m->detector, m->rho, m->stream));
    if (!rc)
        m->hist.flip();                      // the kernel wrote the other slots
    return rc;
}
