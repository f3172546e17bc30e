// cmhip_dyn.hip -- the dynamics stage on the host side (include/coolmic_hip.h, "dynamics"): the object beside the
// batch, its validation, the launch of k_dyn.hip's kernels (the keyed ones while a side-chain key is set, the RMS
// ones for an object with the RMS detector), the curves, the keys, reset, the gain meter and the curve designers.
//
// Device state of a dynamics stage: one curve of DYN_CURVE uint16 entries per stream, the streams' history, int16
// [2][S][halo * C] raw input frames, two slots selected by a parity the host flips per run (HistoryPair,
// csrc/cmhip_stage.h), the meter, uint32 [S], and the key map, uint32 [S]: the stream whose level steers stream s,
// s itself where no key is set.  The host keeps a mirror of the curves and of the map; cmhip_dyn_get_curve and
// cmhip_dyn_get_key answer from them, and the mirror's count of keyed streams chooses a run's kernels.  A new curve or
// key reaches the device inside a kernel's arguments (k_dyn_set, k_dynk_set), so it is ordered with the runs by the
// stream alone and no staging memory outlives the call.
#include "cmhip_engine.h"

#include <math.h>
#include <string.h>

constexpr uint64_t DYN_MAX_SAMPLES = 1ull << 31;     // per slot and run: the kernels index a slot in 32 bits

struct cmhip_dyn : StageBase {
    cmhip_dyn_desc_t d;
    DynGeom g;
    uint32_t detector;                 // DYN_DETECT_*, fixed at creation
    uint16_t *d_curve;
    uint32_t *d_gmin;
    HistoryPair hist;                  // [2][S][halo * C]
    uint32_t *d_key;
    std::vector<uint16_t> curve;       // the mirror: [S][DYN_CURVE]
    std::vector<uint32_t> key;         // the mirror: [S], s where stream s follows its own level
    size_t keyed;                      // streams of the mirror with key[s] != s
};

static_assert(CMHIP_DYN_CURVE == DYN_CURVE, "the header's curve length is the kernels'");
static_assert(CMHIP_DYN_DETECT_MEAN == DYN_DETECT_MEAN && CMHIP_DYN_DETECT_RMS == DYN_DETECT_RMS,
              "the header's detectors are the kernels'");

extern "C" int cmhip_dyn_check(unsigned detector_log2, unsigned smooth_log2, unsigned hold)
{
    if (!dyn_geom(detector_log2, smooth_log2, hold, nullptr))
        return fail(COOLMIC_ERROR_INVAL, "dyn: detector_log2 %u, smooth_log2 %u, hold %u: 3..10, 3..9, and "
                    "2^smooth_log2 + hold <= 2048", detector_log2, smooth_log2, hold);
    return COOLMIC_ERROR_NONE;
}

extern "C" int cmhip_dyn_check_detector(unsigned detector, unsigned detector_log2, unsigned smooth_log2, unsigned hold)
{
    if (detector > DYN_DETECT_RMS)
        return fail(COOLMIC_ERROR_INVAL, "dyn: detector %u: 0 (mean magnitude) or 1 (RMS)", detector);
    return cmhip_dyn_check(detector_log2, smooth_log2, hold);
}

// test hook: what cmhip_dyn_set_curve asks of a table (host logic, needs no GPU)
extern "C" int cmhip_test_dyn_curve_ok(const uint16_t *curve) { return curve && dyn_curve_ok(curve) ? 1 : 0; }

// ---------------------------------------------------------------------------
// the curve designer (host only)

extern "C" int cmhip_dyn_design(const cmhip_dyn_curve_desc_t *c, uint16_t *curve)
{
    if (!c || !curve)
        return fail(COOLMIC_ERROR_FAULT, "dyn_design: NULL argument");
    const double ct = c->comp_threshold_db, R = c->comp_ratio, K = c->comp_knee_db;
    const double gt = c->gate_threshold_db, Re = c->gate_ratio, rng = c->gate_range_db;
    if (!isfinite(ct) || !isfinite(R) || !isfinite(K) || !isfinite(gt) || !isfinite(Re) || !isfinite(rng))
        return fail(COOLMIC_ERROR_INVAL, "dyn_design: every parameter must be finite");
    if (R < 1.0 || Re < 1.0 || K < 0.0 || rng < 0.0)
        return fail(COOLMIC_ERROR_INVAL, "dyn_design: ratios must be at least 1, knee and range at least 0 dB");
    auto entry = [](double db) {
        const double q = floor(32768.0 * pow(10.0, db / 20.0) + 0.5);
        return (uint16_t)(q < 32768.0 ? q : 32768.0);
    };
    curve[0] = entry(-rng);                          // silence: the gate's full range
    for (unsigned k = 1; k < DYN_CURVE_USED; k++) {
        const double v = ldexp((double)(8u + (k - 1u) % 8u), (int)((k - 1u) / 8u) - 3);      // the knot's level
        const double x = 20.0 * log10(v / 32768.0), d = x - ct;
        double comp;
        if (2.0 * d < -K)
            comp = 0.0;
        else if (K > 0.0 && 2.0 * fabs(d) <= K)
            comp = (1.0 / R - 1.0) * (d + K / 2.0) * (d + K / 2.0) / (2.0 * K);
        else
            comp = (1.0 / R - 1.0) * d;
        double gate = 0.0;
        if (rng > 0.0 && x < gt)
            gate = fmax(-rng, (x - gt) * (Re - 1.0));
        curve[k] = entry(comp + gate);
    }
    for (unsigned k = DYN_CURVE_USED; k < DYN_CURVE; k++)
        curve[k] = 0;
    return COOLMIC_ERROR_NONE;
}

// a duck curve: unity below the threshold, depth_db down above it, a linear knee (in dB) between
extern "C" int cmhip_dyn_design_duck(const cmhip_dyn_duck_desc_t *c, uint16_t *curve)
{
    if (!c || !curve)
        return fail(COOLMIC_ERROR_FAULT, "dyn_design_duck: NULL argument");
    const double th = c->threshold_db, depth = c->depth_db, K = c->knee_db;
    if (!isfinite(th) || !isfinite(depth) || !isfinite(K))
        return fail(COOLMIC_ERROR_INVAL, "dyn_design_duck: every parameter must be finite");
    if (depth < 0.0 || K < 0.0)
        return fail(COOLMIC_ERROR_INVAL, "dyn_design_duck: depth and knee must be at least 0 dB");
    curve[0] = (uint16_t)DYN_UNITY;                  // silence: nothing to duck under
    for (unsigned k = 1; k < DYN_CURVE_USED; k++) {
        const double v = ldexp((double)(8u + (k - 1u) % 8u), (int)((k - 1u) / 8u) - 3);      // the knot's level
        const double x = 20.0 * log10(v / 32768.0), d = x - th;
        double g;
        if (K > 0.0)
            g = -depth * fmin(fmax((d + K / 2.0) / K, 0.0), 1.0);
        else
            g = d >= 0.0 ? -depth : 0.0;
        const double q = floor(32768.0 * pow(10.0, g / 20.0) + 0.5);
        curve[k] = (uint16_t)(q < 32768.0 ? q : 32768.0);
    }
    for (unsigned k = DYN_CURVE_USED; k < DYN_CURVE; k++)
        curve[k] = 0;
    return COOLMIC_ERROR_NONE;
}

// ---------------------------------------------------------------------------
// the object

static int dyn_init(cmhip_dyn_t *m)
{
    const cmhip_dyn_desc_t &d = m->d;
    const size_t S = d.streams;
    if (m->open("dyn_new", d.device, d.hip_stream, S) || m->array("dyn_new", &m->d_curve, S * DYN_CURVE) ||
        m->array("dyn_new", &m->d_gmin, S, DYN_UNITY) || m->array("dyn_new", &m->d_key, S) ||
        m->hist.init(*m, "dyn_new", S, (size_t)m->g.halo * d.channels))
        return COOLMIC_ERROR_GENERIC;
    m->curve.assign(S * DYN_CURVE, (uint16_t)DYN_UNITY);         // at creation: unity everywhere, a pure delay
    if (stage_launched("dyn_new", launch_dyn_set(m->d_curve, 0, d.streams, m->curve.data(), m->stream)))
        return COOLMIC_ERROR_GENERIC;
    m->key.resize(S);                                            // at creation: every stream is its own key
    for (size_t s = 0; s < S; s++)
        m->key[s] = (uint32_t)s;
    m->keyed = 0;
    return stage_launched("dyn_new", launch_dyn_set_key(m->d_key, 0, d.streams, 0, true, m->stream));
}

extern "C" void cmhip_dyn_free(cmhip_dyn_t *m) { stage_free(m); }

extern "C" cmhip_dyn_t *cmhip_dyn_new_detector(const cmhip_dyn_desc_t *d, unsigned detector)
{
    if (!d) {
        fail(COOLMIC_ERROR_FAULT, "dyn_new: NULL argument");
        return nullptr;
    }
    if (detector > DYN_DETECT_RMS) {
        fail(COOLMIC_ERROR_INVAL, "dyn_new: detector %u: 0 (mean magnitude) or 1 (RMS)", detector);
        return nullptr;
    }
    DynGeom g;
    if (d->streams == 0 || d->channels == 0 || d->channels > MAX_CH || d->max_frames == 0 ||
        !dyn_geom(d->detector_log2, d->smooth_log2, d->hold, &g)) {
        fail(COOLMIC_ERROR_INVAL, "dyn_new: streams, channels (1..16) and max_frames must be positive, detector_log2 in "
             "3..10, smooth_log2 in 3..9 and 2^smooth_log2 + hold <= 2048");
        return nullptr;
    }
    if (d->max_frames > DYN_MAX_SAMPLES / d->channels) {
        fail(COOLMIC_ERROR_INVAL, "dyn_new: max_frames %zu: a slot of a run would pass 2^31 samples", d->max_frames);
        return nullptr;
    }
    if ((uint64_t)d->streams * g.halo * d->channels >= (1ull << 31)) {
        fail(COOLMIC_ERROR_INVAL, "dyn_new: %u streams: the history would pass 2^31 samples", d->streams);
        return nullptr;
    }
    return stage_new<cmhip_dyn>("dyn_new", [&](cmhip_dyn_t *m) {
        m->d = *d;
        m->g = g;
        m->detector = detector;
        return dyn_init(m);
    });
}

extern "C" cmhip_dyn_t *cmhip_dyn_new(const cmhip_dyn_desc_t *d) { return cmhip_dyn_new_detector(d, DYN_DETECT_MEAN); }

extern "C" unsigned cmhip_dyn_detector(const cmhip_dyn_t *m) { return m ? m->detector : 0u; }

extern "C" unsigned cmhip_dyn_delay(const cmhip_dyn_t *m) { return m ? m->g.D : 0u; }

extern "C" int cmhip_dyn_set_curve(cmhip_dyn_t *m, long stream, const uint16_t *curve)
{
    if (!curve)
        return fail(COOLMIC_ERROR_FAULT, "dyn_set_curve: NULL argument");
    StreamRange sr;
    int rc = stage_streams(m, "dyn_set_curve", stream, &sr);
    if (rc)
        return rc;
    if (!dyn_curve_ok(curve))
        return fail(COOLMIC_ERROR_INVAL, "dyn_set_curve: an entry of 0..%u is above 32768", DYN_CURVE_USED - 1u);
    HIP_TRY(hipSetDevice(m->d.device));
    rc = stage_launched("dyn_set_curve", launch_dyn_set(m->d_curve, sr.lo, sr.n, curve, m->stream));
    if (rc)
        return rc;
    for (size_t s = sr.lo; s < (size_t)sr.lo + sr.n; s++)
        memcpy(&m->curve[s * DYN_CURVE], curve, DYN_CURVE * sizeof(uint16_t));
    return COOLMIC_ERROR_NONE;
}

extern "C" int cmhip_dyn_get_curve(const cmhip_dyn_t *m, unsigned stream, uint16_t *curve)
{
    if (!m || !curve)
        return fail(COOLMIC_ERROR_FAULT, "dyn_get_curve: NULL argument");
    if (stream >= m->d.streams)
        return fail(COOLMIC_ERROR_INVAL, "dyn_get_curve: stream %u out of range", stream);
    memcpy(curve, &m->curve[(size_t)stream * DYN_CURVE], DYN_CURVE * sizeof(uint16_t));
    return COOLMIC_ERROR_NONE;
}

extern "C" int cmhip_dyn_set_key(cmhip_dyn_t *m, long stream, long key)
{
    StreamRange sr;
    int rc = stage_streams(m, "dyn_set_key", stream, &sr);
    if (rc)
        return rc;
    if (key < -1 || (key >= 0 && (unsigned long)key >= m->d.streams))
        return fail(COOLMIC_ERROR_INVAL, "dyn_set_key: key %ld out of range", key);
    HIP_TRY(hipSetDevice(m->d.device));
    const bool own = key < 0;
    rc = stage_launched("dyn_set_key", launch_dyn_set_key(m->d_key, sr.lo, sr.n, own ? 0u : (uint32_t)key, own, m->stream));
    if (rc)
        return rc;
    for (size_t s = sr.lo; s < (size_t)sr.lo + sr.n; s++) {
        const uint32_t k = own ? (uint32_t)s : (uint32_t)key;
        if (m->key[s] != s)
            m->keyed--;
        if (k != s)
            m->keyed++;
        m->key[s] = k;
    }
    return COOLMIC_ERROR_NONE;
}

extern "C" int cmhip_dyn_get_key(const cmhip_dyn_t *m, unsigned stream, long *key)
{
    if (!m || !key)
        return fail(COOLMIC_ERROR_FAULT, "dyn_get_key: NULL argument");
    if (stream >= m->d.streams)
        return fail(COOLMIC_ERROR_INVAL, "dyn_get_key: stream %u out of range", stream);
    *key = m->key[stream] == stream ? -1L : (long)m->key[stream];
    return COOLMIC_ERROR_NONE;
}

extern "C" void *cmhip_dyn_hip_stream(cmhip_dyn_t *m) { return m ? (void *)m->stream : nullptr; }

extern "C" int cmhip_dyn_sync(cmhip_dyn_t *m) { return stage_sync(m, "dyn_sync"); }

extern "C" int cmhip_dyn_reset(cmhip_dyn_t *m, long stream)
{
    StreamRange sr;
    const int rc = stage_streams(m, "dyn_reset", stream, &sr);
    if (rc)
        return rc;
    HIP_TRY(hipSetDevice(m->d.device));
    HIP_TRY(m->hist.reset(sr.lo, sr.n, m->stream));
    HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)(m->d_gmin + sr.lo), (int)DYN_UNITY, sr.n, m->stream));
    return COOLMIC_ERROR_NONE;
}

extern "C" int cmhip_dyn_min_gain(cmhip_dyn_t *m, uint32_t *out, int reset)
{
    if (!m || !out)
        return fail(COOLMIC_ERROR_FAULT, "dyn_min_gain: NULL argument");
    return stage_read(m, out, m->d_gmin, m->d.streams * sizeof(uint32_t), reset != 0, DYN_UNITY);
}

extern "C" int cmhip_dyn_run(cmhip_dyn_t *m, const void *in, size_t in_stride, size_t frames,
                             const uint32_t *frames_per_stream, void *out, size_t out_stride)
{
    if (!m)
        return fail(COOLMIC_ERROR_FAULT, "dyn_run: NULL argument");
    const unsigned S = m->d.streams, C = m->d.channels;
    // (the two arrays may not share a byte: a tile reads the frames in front of it again after its neighbour may have
    // written them)
    const StageRun r = {in, out, in_stride, out_stride, frames, m->d.max_frames, frames_per_stream, S, S, C, frames, C,
                        STAGE_APART};
    int rc;
    if (!stage_run_begin(m, "dyn_run", r, &rc))
        return rc;
    if (plan_dyn(S, C, m->g.a, m->g.b, m->g.H, (uint32_t)frames).err)
        return fail(COOLMIC_ERROR_INVAL, "dyn_run: %u streams of %zu frames: the grid would reach 2^31 workgroups", S,
                    frames);
    // a keyed stream and its key advance together: frame n of the one is frame n of the other
    if (frames_per_stream && m->keyed)
        for (unsigned s = 0; s < S; s++) {
            const uint32_t k = m->key[s];
            if (frames_per_stream[s] != frames_per_stream[k])
                return fail(COOLMIC_ERROR_INVAL, "dyn_run: stream %u has %u frames, its key, stream %u, has %u", s,
                            frames_per_stream[s], k, frames_per_stream[k]);
        }
    // nothing was touched so far; from here on the run happens
    DynArgs a;
    memset(&a, 0, sizeof(a));
    a.in = (const int16_t *)in;
    a.out = (int16_t *)out;
    a.curve = m->d_curve;
    a.hist = m->hist.d;
    a.gmin = m->d_gmin;
    a.in_stride = in_stride;
    a.out_stride = out_stride;
    a.frames = (uint32_t)frames;
    a.streams = S;
    a.channels = C;
    a.parity = m->hist.parity();
    a.a = m->g.a;
    a.b = m->g.b;
    a.W = m->g.W;
    HIP_TRY(m->send_counts(frames_per_stream, S, &a.nframes));
    // (the keyed kernels only while a key is set)
    rc = stage_launched("dyn_run", launch_dyn(a, m->detector, m->keyed ? m->d_key : nullptr, m->stream));
    if (!rc)
        m->hist.flip();                      // the kernel wrote the other slots
    return rc;
}
