// cmhip_bus.hip -- the mix bus on the host side (include/coolmic_hip.h, "mix bus"): the bus object beside the batch,
// its validation, the routing table's way to the device, the launch of k_bus.hip's kernels, the table check and the
// mix-minus table.
//
// Device state of a bus: the routing table in the kernels' form (csrc/bus_route.h compiles it) -- first[B+1],
// send[max_sends], wk[max_sends][C_out][CP] in one array -- and the counts of a run, [S] per stream and [B] per bus.
// That is all: there is no history.  The host keeps the table as the caller gave it (cmhip_bus_get_routing) and as
// compiled (a run's out_frames come from it without a device wait).
//
// Both travel by hipMemcpyAsync on the object's stream from PINNED memory the object owns, so they are ordered with the
// runs by the stream alone and nothing the caller owns is read after a call returns: the table from one staging area
// with an event (a second set waits on the host until the first one's copy has executed), a run's counts from a small
// ring of blocks with an event each (CountsRing, csrc/cmhip_stage.h: run COUNTS_RING + 1 waits for run 1's copy).
//
// Send ramps (include/coolmic_hip.h, "send ramps"): the first cmhip_bus_ramp_sends that ramps allocates a record per
// send on the device (BusRampArgs::ramp), a pinned copy of them beside the table's staging area, and the host's
// mirror (csrc/bus_ramp.h).  Every cmhip_bus_ramp_sends compiles the table again -- the group split from both ends of
// every running ramp -- and sends the WHOLE table and every record through the staging path: the split of a bus may
// move at any of its sends, and one copy of the whole is simpler to order than patches (DESIGN 4.12 has the size).
// The host sees every run's counts, so the mirror advances as the device does and knows whether any send ramps: only
// then does cmhip_bus_run launch k_busramp.hip's kernels, and a bus that never ramps launches what it always did.
#include "cmhip_engine.h"

#include <stdlib.h>
#include <string.h>

#include <memory>

#include "bus_ramp.h"
#include "bus_route.h"

constexpr uint64_t BUS_MAX_SAMPLES = 1ull << 31;     // per slot and run: the kernels index a slot in 32 bits

struct cmhip_bus : StageBase {         // d_counts and its ring hold [S] streams | [B] buses
    cmhip_bus_desc_t d;
    uint32_t *d_table;                 // first[B+1] | send[max_sends] | wk[max_sends * NW]
    uint32_t *h_table;                 // pinned, the same layout
    hipEvent_t table_ev;
    bool table_busy;                   // a copy from h_table was queued and not yet waited for
    bool nt_loads;
    std::vector<uint32_t> bus, strm;   // the mirror, in the caller's order
    std::vector<int16_t> w;
    BusTable t;                        // ... and compiled
    uint32_t *d_ramp;                  // the sends' ramp records in compiled order, allocated by the first ramp
    uint32_t *h_ramp;                  // pinned, the same layout: staged with the table, under table_ev
    std::unique_ptr<BusRampMirror> ramp;       // ... and their mirror, in the caller's order
    std::vector<uint32_t> pos;         // compiled position of the caller's send j (while ramp != nullptr)
    std::vector<uint32_t> bound;       // the split's bounds [n][C_out] (scratch of a compile)
    std::vector<uint32_t> bus_count;   // a ramp run's count per bus (scratch of a run)

    // the pinned staging blocks and their event are the bus's own (stage_free: behind close(), the device current)
    ~cmhip_bus()
    {
        (void)hipHostFree(h_table);
        (void)hipHostFree(h_ramp);
        if (table_ev)
            (void)hipEventDestroy(table_ev);
    }
};

static size_t bus_nw(const cmhip_bus_t *m) { return (size_t)m->d.channels_out * ((m->d.channels_in + 1) / 2); }

static int bus_route_fail(const char *who, BusRouteError e, size_t where)
{
    switch (e) {
    case BUS_ROUTE_OK: return COOLMIC_ERROR_NONE;
    case BUS_ROUTE_GEOMETRY:
        return fail(COOLMIC_ERROR_INVAL, "%s: buses and streams must be positive, both channel counts in 1..16", who);
    case BUS_ROUTE_SIZE: return fail(COOLMIC_ERROR_INVAL, "%s: the table would reach 2^31 entries", who);
    case BUS_ROUTE_NULL: return fail(COOLMIC_ERROR_FAULT, "%s: NULL argument", who);
    case BUS_ROUTE_BUS: return fail(COOLMIC_ERROR_INVAL, "%s: send %zu: bus out of range", who, where);
    case BUS_ROUTE_STREAM: return fail(COOLMIC_ERROR_INVAL, "%s: send %zu: stream out of range", who, where);
    case BUS_ROUTE_ROW: return fail(COOLMIC_ERROR_INVAL, "%s: send %zu has a row with sum |w| above 65535", who, where);
    }
    return fail(COOLMIC_ERROR_GENERIC, "%s: unknown error", who);
}

extern "C" int cmhip_bus_check(unsigned buses, unsigned streams, unsigned channels_in, unsigned channels_out, size_t n,
                               const uint32_t *bus, const uint32_t *stream, const int16_t *W)
{
    size_t where = 0;
    return bus_route_fail("bus_check", bus_route_check(buses, streams, channels_in, channels_out, n, bus, stream, W, &where),
                          where);
}

extern "C" int cmhip_bus_mix_minus(unsigned n, int16_t w, uint32_t *bus, uint32_t *stream, int16_t *W, size_t cap_sends,
                                   unsigned channels)
{
    if (n == 0 || channels == 0 || channels > MAX_CH)
        return fail(COOLMIC_ERROR_INVAL, "bus_mix_minus: %u participants of %u channels", n, channels);
    const size_t sends = (size_t)n * (n - 1);
    if (cap_sends < sends)
        return fail(COOLMIC_ERROR_INVAL, "bus_mix_minus: room for %zu sends, the table has %zu", cap_sends, sends);
    if (sends && (!bus || !stream || !W))
        return fail(COOLMIC_ERROR_FAULT, "bus_mix_minus: NULL argument");
    size_t j = 0;
    for (unsigned b = 0; b < n; b++) {
        for (unsigned s = 0; s < n; s++) {
            if (s == b)
                continue;
            bus[j] = b;
            stream[j] = s;
            int16_t *m = W + j * channels * channels;
            memset(m, 0, (size_t)channels * channels * sizeof(int16_t));
            for (unsigned c = 0; c < channels; c++)
                m[c * channels + c] = w;
            j++;
        }
    }
    return COOLMIC_ERROR_NONE;
}

// test hook: the compiled form of a table -- first [B+1], stream [n], flag [n], wk [n][C_out][CP] (host logic, no GPU)
extern "C" int cmhip_test_bus_compile(unsigned buses, unsigned streams, unsigned channels_in, unsigned channels_out,
                                      size_t n, const uint32_t *bus, const uint32_t *stream, const int16_t *W,
                                      uint32_t *first, uint32_t *stream_out, uint32_t *flag, uint32_t *wk)
{
    const int rc = cmhip_bus_check(buses, streams, channels_in, channels_out, n, bus, stream, W);
    if (rc)
        return rc;
    BusTable t;
    bus_route_compile(buses, channels_in, channels_out, n, bus, stream, W, t);
    memcpy(first, t.first.data(), t.first.size() * sizeof(uint32_t));
    if (n) {
        memcpy(stream_out, t.stream.data(), n * sizeof(uint32_t));
        memcpy(flag, t.flag.data(), n * sizeof(uint32_t));
        memcpy(wk, t.wk.data(), t.wk.size() * sizeof(uint32_t));
    }
    return COOLMIC_ERROR_NONE;
}

static int bus_init(cmhip_bus_t *m)
{
    const cmhip_bus_desc_t &d = m->d;
    const size_t B = d.buses, S = d.streams, words = B + 1 + d.max_sends * (1 + bus_nw(m));
    if (m->open("bus_new", d.device, d.hip_stream, S + B) || m->array("bus_new", &m->d_table, words))
        return COOLMIC_ERROR_GENERIC;
    HIP_TRY(hipHostMalloc((void **)&m->h_table, words * sizeof(uint32_t), hipHostMallocDefault));
    HIP_TRY(hipEventCreateWithFlags(&m->table_ev, hipEventDisableTiming));
    m->bus_count.assign(B, 0);
    // routing at creation: empty
    bus_route_compile(d.buses, d.channels_in, d.channels_out, 0, nullptr, nullptr, nullptr, m->t);
    return COOLMIC_ERROR_NONE;
}

extern "C" void cmhip_bus_free(cmhip_bus_t *m) { stage_free(m); }

extern "C" cmhip_bus_t *cmhip_bus_new(const cmhip_bus_desc_t *d)
{
    if (!d) {
        fail(COOLMIC_ERROR_FAULT, "bus_new: NULL argument");
        return nullptr;
    }
    if (d->streams == 0 || d->buses == 0 || d->channels_in < 1 || d->channels_in > MAX_CH || d->channels_out < 1 ||
        d->channels_out > MAX_CH || d->max_frames == 0 || d->max_sends == 0) {
        fail(COOLMIC_ERROR_INVAL,
             "bus_new: streams, buses, channels_in, channels_out (1..16), max_frames and max_sends must be positive");
        return nullptr;
    }
    const unsigned cmax = d->channels_in > d->channels_out ? d->channels_in : d->channels_out;
    if (d->max_frames >= BUS_MAX_SAMPLES || d->max_frames * cmax >= BUS_MAX_SAMPLES) {
        fail(COOLMIC_ERROR_INVAL, "bus_new: max_frames %zu: a slot of a run would reach 2^31 samples", d->max_frames);
        return nullptr;
    }
    if (bus_route_check(d->buses, d->streams, d->channels_in, d->channels_out, d->max_sends, nullptr, nullptr, nullptr,
                        nullptr) == BUS_ROUTE_SIZE) {
        fail(COOLMIC_ERROR_INVAL, "bus_new: %u streams, %u buses, %zu sends: the table would reach 2^31 entries",
             d->streams, d->buses, d->max_sends);
        return nullptr;
    }
    return stage_new<cmhip_bus>("bus_new", [&](cmhip_bus_t *m) {
        m->d = *d;
        return bus_init(m);
    });
}

// The table in force (m->bus, m->strm, m->w) compiled and on its way to the device; the caller has waited for the
// staging area.  With ramp state the group split comes from the mirror's bounds -- for sends at rest these are their
// own row sums, and the result is bus_route_compile's -- and `records` sends every send's record behind the table.
static int bus_upload(cmhip_bus_t *m, bool records)
{
    const unsigned B = m->d.buses, CI = m->d.channels_in, CO = m->d.channels_out;
    const size_t n = m->bus.size();
    if (m->ramp) {
        bus_ramp_bounds(*m->ramp, CI, CO, m->bound);
        bus_route_compile_bounds(B, CI, CO, n, m->bus.data(), m->strm.data(), m->w.data(), m->bound.data(), m->t, &m->pos);
    } else {
        bus_route_compile(B, CI, CO, n, m->bus.data(), m->strm.data(), m->w.data(), m->t);
    }
    const size_t nw = bus_nw(m), send0 = (size_t)B + 1, wk0 = send0 + m->d.max_sends;
    for (unsigned b = 0; b <= B; b++)
        m->h_table[b] = bus_first_word(m->t, b);
    for (size_t p = 0; p < n; p++)
        m->h_table[send0 + p] = bus_send_word(m->t, p);
    if (n)
        memcpy(m->h_table + wk0, m->t.wk.data(), n * nw * sizeof(uint32_t));
    HIP_TRY(hipMemcpyAsync(m->d_table, m->h_table, (send0 + n) * sizeof(uint32_t), hipMemcpyHostToDevice, m->stream));
    m->table_busy = true;                            // (whatever follows: the area may be in use)
    if (n)
        HIP_TRY(hipMemcpyAsync(m->d_table + wk0, m->h_table + wk0, n * nw * sizeof(uint32_t), hipMemcpyHostToDevice,
                               m->stream));
    if (records && n) {
        const size_t recw = bus_ramp_record_dwords(CI, CO);
        for (size_t j = 0; j < n; j++)
            m->ramp->record(j, CI, CO, m->h_ramp + m->pos[j] * recw);
        HIP_TRY(hipMemcpyAsync(m->d_ramp, m->h_ramp, n * recw * sizeof(uint32_t), hipMemcpyHostToDevice, m->stream));
    }
    HIP_TRY(hipEventRecord(m->table_ev, m->stream));
    return COOLMIC_ERROR_NONE;
}

extern "C" int cmhip_bus_set_routing(cmhip_bus_t *m, size_t n, const uint32_t *bus, const uint32_t *stream,
                                     const int16_t *W)
{
    if (!m)
        return fail(COOLMIC_ERROR_FAULT, "bus_set_routing: NULL argument");
    if (n > m->d.max_sends)
        return fail(COOLMIC_ERROR_INVAL, "bus_set_routing: %zu sends above max_sends %zu", n, m->d.max_sends);
    const unsigned B = m->d.buses, CI = m->d.channels_in, CO = m->d.channels_out;
    size_t where = 0;
    const BusRouteError e = bus_route_check(B, m->d.streams, CI, CO, n, bus, stream, W, &where);
    if (e != BUS_ROUTE_OK)
        return bus_route_fail("bus_set_routing", e, where);
    HIP_TRY(hipSetDevice(m->d.device));
    if (m->table_busy) {                             // the staging area is still the source of the last set's copy
        HIP_TRY(hipEventSynchronize(m->table_ev));
        m->table_busy = false;
    }
    return stage_guard("bus_set_routing", [&] {
        if (m->ramp)                                 // every ramp ends: all sends at rest on the new table
            m->ramp->init(n, (size_t)CO * CI, bus, W);
        // nothing of the table was touched so far; from here on it changes
        m->bus.assign(bus, bus + n);
        m->strm.assign(stream, stream + n);
        m->w.assign(W, W + n * CO * CI);
        return bus_upload(m, false);
    });
}

extern "C" size_t cmhip_bus_sends(const cmhip_bus_t *m) { return m ? m->bus.size() : 0; }

extern "C" int cmhip_bus_get_routing(const cmhip_bus_t *m, size_t cap, uint32_t *bus, uint32_t *stream, int16_t *W)
{
    if (!m)
        return fail(COOLMIC_ERROR_FAULT, "bus_get_routing: NULL argument");
    const size_t n = m->bus.size();
    if (cap < n)
        return fail(COOLMIC_ERROR_INVAL, "bus_get_routing: room for %zu sends, the table has %zu", cap, n);
    if (n && (!bus || !stream || !W))
        return fail(COOLMIC_ERROR_FAULT, "bus_get_routing: NULL argument");
    if (n) {
        memcpy(bus, m->bus.data(), n * sizeof(uint32_t));
        memcpy(stream, m->strm.data(), n * sizeof(uint32_t));
        memcpy(W, m->w.data(), m->w.size() * sizeof(int16_t));
    }
    return COOLMIC_ERROR_NONE;
}

// the ramp records, their staging copy and the mirror, on first use: every send at rest on its matrix
static int bus_ramp_alloc(cmhip_bus_t *m)
{
    return stage_guard("bus_ramp_sends", [&] {
        const unsigned CI = m->d.channels_in, CO = m->d.channels_out;
        const size_t words = m->d.max_sends * bus_ramp_record_dwords(CI, CO);
        auto mirror = std::make_unique<BusRampMirror>();
        mirror->init(m->bus.size(), (size_t)CO * CI, m->bus.data(), m->w.data());
        if (!m->h_ramp && hipHostMalloc((void **)&m->h_ramp, words * sizeof(uint32_t), hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            m->h_ramp = nullptr;
            return fail(COOLMIC_ERROR_NOMEM, "bus_ramp_sends: no pinned memory for %zu bytes", words * sizeof(uint32_t));
        }
        const int rc = m->array("bus_ramp_sends", &m->d_ramp, words);
        if (!rc)
            m->ramp = std::move(mirror);
        return rc;
    });
}

extern "C" int cmhip_bus_ramp_sends(cmhip_bus_t *m, size_t first, size_t count, const int16_t *W, uint32_t ramp_frames)
{
    if (!m || (count && !W))
        return fail(COOLMIC_ERROR_FAULT, "bus_ramp_sends: NULL argument");
    const size_t n = m->bus.size();
    if (first > n || count > n - first)
        return fail(COOLMIC_ERROR_INVAL, "bus_ramp_sends: sends %zu .. %zu + %zu: the table has %zu", first, first, count, n);
    if (ramp_frames > MIX_RAMP_MAX)
        return fail(COOLMIC_ERROR_INVAL, "bus_ramp_sends: %u frames above %u", ramp_frames, MIX_RAMP_MAX);
    if (count == 0)
        return COOLMIC_ERROR_NONE;
    const unsigned CI = m->d.channels_in, CO = m->d.channels_out;
    const size_t e = (size_t)CO * CI;
    for (size_t j = 0; j < count; j++)
        for (unsigned o = 0; o < CO; o++) {
            uint32_t sum = 0;
            for (unsigned c = 0; c < CI; c++)
                sum += bus_abs16(W[j * e + o * CI + c]);
            if (sum > BUS_ROW_MAX)
                return fail(COOLMIC_ERROR_INVAL, "bus_ramp_sends: send %zu has a row with sum |w| above 65535", first + j);
        }
    HIP_TRY(hipSetDevice(m->d.device));
    if (ramp_frames >= 2 && !m->ramp) {
        const int rc = bus_ramp_alloc(m);
        if (rc)
            return rc;
    }
    if (m->table_busy) {                             // the staging area is still the source of the last table's copy
        HIP_TRY(hipEventSynchronize(m->table_ev));
        m->table_busy = false;
    }
    // nothing of the table was touched so far; from here on it changes
    for (size_t j = 0; j < count; j++) {
        if (ramp_frames >= 2)
            m->ramp->start(first + j, W + j * e, ramp_frames);
        else if (m->ramp)
            m->ramp->step(first + j, W + j * e);
        memcpy(&m->w[(first + j) * e], W + j * e, e * sizeof(int16_t));
    }
    return bus_upload(m, m->ramp != nullptr);
}

extern "C" int cmhip_bus_ramp_state(const cmhip_bus_t *m, size_t send, uint32_t *done, uint32_t *ramp_frames,
                                    int16_t *W_now)
{
    if (!m || !done || !ramp_frames)
        return fail(COOLMIC_ERROR_FAULT, "bus_ramp_state: NULL argument");
    if (send >= m->bus.size())
        return fail(COOLMIC_ERROR_INVAL, "bus_ramp_state: send %zu out of range", send);
    const size_t e = (size_t)m->d.channels_out * m->d.channels_in;
    if (m->ramp && m->ramp->ramping(send)) {
        *done = m->ramp->r.done[send];
        *ramp_frames = m->ramp->r.R[send];
        if (W_now)
            m->ramp->now(send, W_now);
    } else {
        *done = *ramp_frames = 0;
        if (W_now)
            memcpy(W_now, &m->w[send * e], e * sizeof(int16_t));
    }
    return COOLMIC_ERROR_NONE;
}

extern "C" void *cmhip_bus_hip_stream(cmhip_bus_t *m) { return m ? (void *)m->stream : nullptr; }

extern "C" int cmhip_bus_sync(cmhip_bus_t *m) { return stage_sync(m, "bus_sync"); }

// test hook (tools/bench_bus.py): k_bus_fast's input loads non-temporal (on != 0) or plain (the default)
extern "C" void cmhip_test_bus_nt_loads(cmhip_bus_t *m, int on)
{
    if (m)
        m->nt_loads = on != 0;
}

extern "C" int cmhip_bus_run(cmhip_bus_t *m, const void *in, size_t in_stride, size_t frames,
                             const uint32_t *frames_per_stream, void *out, size_t out_stride, uint32_t *out_frames)
{
    if (!m)
        return fail(COOLMIC_ERROR_FAULT, "bus_run: NULL argument");
    const unsigned S = m->d.streams, B = m->d.buses, CI = m->d.channels_in, CO = m->d.channels_out;
    const StageRun r = {in, out, in_stride, out_stride, frames, m->d.max_frames, frames_per_stream, S, B, CI, frames, CO,
                        STAGE_APART};
    int rc;
    const bool go = stage_run_begin(m, "bus_run", r, &rc);
    if (rc)
        return rc;
    BusArgs a;
    memset(&a, 0, sizeof(a));
    a.in = (const int16_t *)in;
    a.out = (int16_t *)out;
    a.nframes = m->counts_arg(frames_per_stream);
    a.bus_frames = m->d_counts + S;
    a.first = m->d_table;
    a.send = m->d_table + B + 1;
    a.wk = a.send + m->d.max_sends;
    a.in_stride = in_stride;
    a.out_stride = out_stride;
    a.frames = (uint32_t)frames;
    a.buses = B;
    a.channels_in = CI;
    a.channels_out = CO;
    a.nt_loads = m->nt_loads ? 1u : 0u;
    const bool ramps = m->ramp && m->ramp->any();    // (the ramp kernels' tile may be the finer one)
    if (go && (ramps ? plan_busramp(a) : plan_bus(a)).err != hipSuccess)
        return fail(COOLMIC_ERROR_INVAL, "bus_run: %u buses of %zu frames: the grid would reach 2^31 workgroups", B,
                    frames);
    // nothing was touched so far; from here on the run happens
    if (out_frames)
        for (unsigned b = 0; b < B; b++)
            out_frames[b] = bus_out_frames(m->t, b, frames_per_stream, (uint32_t)frames);
    if (!go || m->bus.empty())
        return COOLMIC_ERROR_NONE;
    if (frames_per_stream) {
        uint32_t *h;
        HIP_TRY(m->counts.take(&h));
        memcpy(h, frames_per_stream, S * sizeof(uint32_t));
        for (unsigned b = 0; b < B; b++)
            h[S + b] = bus_out_frames(m->t, b, frames_per_stream, (uint32_t)frames);
        HIP_TRY(m->counts.send(m->d_counts, (size_t)S + B, m->stream));
    }
    if (!ramps)                                      // nobody ramps: the plain kernels, as ever
        return stage_launched("bus_run", launch_bus(a, m->stream));
    // somebody ramps: the ramp kernels, then every ramping send moves on by its bus's count, there and here
    BusRampArgs ra;
    ra.b = a;
    ra.ramp = m->d_ramp;
    hipError_t e = launch_busramp(ra, m->stream);
    if (e == hipSuccess)
        e = launch_busramp_advance(m->d_ramp, a.nframes ? a.bus_frames : nullptr, a.frames, (uint32_t)m->bus.size(), CI,
                                   CO, m->stream);
    rc = stage_launched("bus_run", e);
    if (rc)
        return rc;
    for (unsigned b = 0; b < B; b++)
        m->bus_count[b] = bus_out_frames(m->t, b, frames_per_stream, (uint32_t)frames);
    m->ramp->advance(m->bus_count.data());
    return COOLMIC_ERROR_NONE;
}
