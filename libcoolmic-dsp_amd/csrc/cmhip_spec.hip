// cmhip_spec.hip -- the spectrum meter of a batch on the host side: the opt-in state, the geometry (block size, band
// table, selected channels), the launch of k_spec.hip's kernel ahead of a run's block kernel, the windows' results with
// the finish in double, and the pieces that need no device (tables, band design, the reference block).
//
// Device state (made by cmhip_batch_set_spectrum(b, 1) for the geometry in force): the windows, 64-bit [S][8][32] band
// sums per stream and selected channel; the streams' last N - 1 transformed samples per selected channel and their
// `back` (csrc/spec_plan.h), each in two slots that the runs alternate between, as true peak keeps its history; the
// tables.  Positions, block counts and the frames a window accounts are mirrored on the host, where every run's counts
// are known.  The VU, true-peak, loudness and correlation windows know nothing of this.  The windows' lifecycle is the
// shared one of csrc/cmhip_meter.h; a window here closes on its completed blocks, not on its frames.
#include "cmhip_engine.h"

#include <math.h>
#include <string.h>

#include <atomic>

// test hook: spectrum passes launched by this process so far
static std::atomic<unsigned long long> g_spec_runs{0};
extern "C" unsigned long long cmhip_debug_spec_count(void) { return g_spec_runs.load(); }

constexpr size_t SPEC_WORDS = SPEC_MAX_CH * SPEC_MAX_BANDS;      // 64-bit words per stream
static_assert(SPEC_MAX_CH == CMHIP_SPEC_MAX_CHANNELS && SPEC_MAX_BANDS == CMHIP_SPEC_MAX_BANDS,
              "the public limits are the kernel's");
static_assert(sizeof(((coolmic_spectrum_result_t *)0)->power) == SPEC_WORDS * 8, "the result holds a whole window");

static bool spec_log2_ok(unsigned n) { return n >= SPEC_MIN_LOG2 && n <= SPEC_MAX_LOG2; }

// ---------------------------------------------------------------------------
// no device needed

extern "C" int cmhip_spec_window(unsigned int fft_log2, int16_t *win)
{
    if (!win)
        return fail(COOLMIC_ERROR_FAULT, "spec_window: NULL argument");
    if (!spec_log2_ok(fft_log2))
        return fail(COOLMIC_ERROR_INVAL, "spec_window: fft_log2 %u outside 8..12", fft_log2);
    spec_window(fft_log2, win);
    return COOLMIC_ERROR_NONE;
}

extern "C" int cmhip_spec_twiddles(unsigned int fft_log2, int32_t *wr, int32_t *wi)
{
    if (!wr || !wi)
        return fail(COOLMIC_ERROR_FAULT, "spec_twiddles: NULL argument");
    if (!spec_log2_ok(fft_log2))
        return fail(COOLMIC_ERROR_INVAL, "spec_twiddles: fft_log2 %u outside 8..12", fft_log2);
    spec_twiddles(fft_log2, wr, wi);
    return COOLMIC_ERROR_NONE;
}

extern "C" int cmhip_spec_design_bands(unsigned int rate, unsigned int fft_log2, unsigned int per_octave,
                                       uint16_t edges[33])
{
    if (!edges)
        return fail(COOLMIC_ERROR_FAULT, "spec_design_bands: NULL argument");
    const int nb = spec_design_bands(rate, fft_log2, per_octave, edges);
    if (nb < 1)
        return fail(COOLMIC_ERROR_INVAL, "spec_design_bands: rate %u, fft_log2 %u, %u per octave: an argument out of "
                    "range or more than 32 bands", rate, fft_log2, per_octave);
    return nb;
}

extern "C" double cmhip_spec_db(uint64_t power, uint64_t blocks) { return spec_db(power, blocks); }

// test hook: the reference block (csrc/spec_plan.h) with the library's tables: x[N] -> p[N / 2 + 1]
extern "C" int cmhip_test_spec_block(unsigned int fft_log2, const int16_t *x, uint64_t *p)
{
    if (!x || !p)
        return COOLMIC_ERROR_FAULT;
    if (!spec_log2_ok(fft_log2))
        return COOLMIC_ERROR_INVAL;
    const size_t N = (size_t)1 << fft_log2;
    std::vector<int16_t> win(N);
    std::vector<int32_t> w(N), z(2 * N);
    spec_window(fft_log2, win.data());
    spec_twiddles(fft_log2, w.data(), w.data() + N / 2);
    spec_block_ref(fft_log2, x, win.data(), w.data(), w.data() + N / 2, z.data(), z.data() + N, p);
    return COOLMIC_ERROR_NONE;
}

// ---------------------------------------------------------------------------
// the batch's meter

static void spec_fill_defaults(cmhip_batch_t *b)
{
    if (b->spec_nb == 0)
        b->spec_nb = spec_default_bands(b->spec_log2, b->spec_edges);
    if (b->spec_nch == 0) {
        b->spec_nch = b->d.channels >= 2 ? 2u : 1u;
        b->spec_ch[0] = 0;
        b->spec_ch[1] = 1;
    }
}

extern "C" int cmhip_batch_spec_configure(cmhip_batch_t *b, unsigned int fft_log2, unsigned int nb,
                                          const uint16_t *edges, unsigned int nch, const unsigned char *channels)
{
    if (!b || (nb && !edges) || (nch && !channels))
        return fail(COOLMIC_ERROR_FAULT, "spec_configure: NULL argument");
    if (b->spec.on)
        return fail(COOLMIC_ERROR_BUSY, "spec_configure: the spectrum is on (turn it off first)");
    if (!spec_log2_ok(fft_log2))
        return fail(COOLMIC_ERROR_INVAL, "spec_configure: fft_log2 %u outside 8..12", fft_log2);
    if (nb && !spec_bands_ok(fft_log2, nb, edges))
        return fail(COOLMIC_ERROR_INVAL, "spec_configure: 1 to 32 bands with 0 <= e[0] < e[1] < ... < e[nb] <= N / 2 + 1");
    if (nch > SPEC_MAX_CH)
        return fail(COOLMIC_ERROR_INVAL, "spec_configure: 1 to %u channels", SPEC_MAX_CH);
    for (unsigned i = 0; i < nch; i++) {
        if (channels[i] >= b->d.channels)
            return fail(COOLMIC_ERROR_INVAL, "spec_configure: channel %u of a batch of %u", channels[i], b->d.channels);
        for (unsigned j = 0; j < i; j++)
            if (channels[j] == channels[i])
                return fail(COOLMIC_ERROR_INVAL, "spec_configure: channel %u twice", channels[i]);
    }
    b->spec_log2 = fft_log2;
    b->spec_nb = nb;
    memset(b->spec_edges, 0, sizeof(b->spec_edges));
    if (nb)
        memcpy(b->spec_edges, edges, (nb + 1) * sizeof(uint16_t));
    b->spec_nch = nch;
    memset(b->spec_ch, 0, sizeof(b->spec_ch));
    if (nch)
        memcpy(b->spec_ch, channels, nch);
    spec_fill_defaults(b);
    return COOLMIC_ERROR_NONE;
}

// beside the windows: the defaults, the state and tables for the geometry in force, the state cleared
static int spec_turn_on(cmhip_batch_t *b)
{
    spec_fill_defaults(b);
    const size_t S = b->d.streams, N = (size_t)1 << b->spec_log2;
    const size_t hist_words = 2 * S * b->spec_nch * N, table_words = 2 * N + SPEC_MAX_BANDS + 1;
    if (!b->d_spec_back)
        HIP_TRY(hipMalloc((void **)&b->d_spec_back, 2 * S * sizeof(uint32_t)));
    if (b->spec_hist_words != hist_words) {  // (the geometry changed while the meter was off)
        (void)hipFree(b->d_spec_hist);
        b->d_spec_hist = nullptr;
        b->spec_hist_words = 0;
        HIP_TRY(hipMalloc((void **)&b->d_spec_hist, hist_words * sizeof(int16_t)));
        b->spec_hist_words = hist_words;
    }
    if (b->spec_table_words != table_words) {
        (void)hipFree(b->d_spec_table);
        b->d_spec_table = nullptr;
        b->spec_table_words = 0;
        HIP_TRY(hipMalloc((void **)&b->d_spec_table, table_words * sizeof(int32_t)));
        b->spec_table_words = table_words;
    }
    // the tables: Wr[N / 2], Wi[N / 2], win[N], edges[33]
    std::vector<int32_t> table(table_words, 0);
    std::vector<int16_t> win(N);
    spec_twiddles(b->spec_log2, table.data(), table.data() + N / 2);
    spec_window(b->spec_log2, win.data());
    for (size_t i = 0; i < N; i++)
        table[N + i] = win[i];
    for (unsigned i = 0; i <= b->spec_nb; i++)
        table[2 * N + i] = b->spec_edges[i];
    HIP_TRY(hipMemcpyAsync(b->d_spec_table, table.data(), table_words * sizeof(int32_t), hipMemcpyHostToDevice, b->stream));
    HIP_TRY(hipMemsetAsync(b->d_spec_hist, 0, hist_words * sizeof(int16_t), b->stream));
    HIP_TRY(hipMemsetAsync(b->d_spec_back, 0, 2 * S * sizeof(uint32_t), b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));        // (the table is a local)
    b->spec_parity = 0;
    b->spec_back.assign(S, 0);
    b->spec_blocks.assign(S, 0);
    return COOLMIC_ERROR_NONE;
}

int cmhip_engine_spec_run(cmhip_batch_t *b, const int16_t *in, size_t frames, const uint32_t *frames_per_stream)
{
    SpecArgs a;
    memset(&a, 0, sizeof(a));
    a.in = in;
    a.param = b->d_param;
    a.nframes = frames_per_stream ? b->d_nframes : nullptr;
    a.sums = b->spec.windows<unsigned long long>();
    a.hist = b->d_spec_hist;
    a.back = b->d_spec_back;
    a.table = b->d_spec_table;
    for (unsigned i = 0; i < b->spec_nch; i++)
        a.chpack |= (uint64_t)b->spec_ch[i] << (8u * i);
    a.frames = (uint32_t)frames;
    a.streams = b->d.streams;
    a.channels = b->d.channels;
    a.log2n = b->spec_log2;
    a.nch = b->spec_nch;
    a.nb = b->spec_nb;
    a.parity = b->spec_parity;
    a.stride = b->stride;
    uint32_t max_blocks = 0;
    for (unsigned s = 0; s < b->d.streams; s++) {
        const uint32_t f = frames_per_stream ? frames_per_stream[s] : (uint32_t)frames;
        const uint32_t nb = spec_run_blocks(b->spec_log2, b->spec_back[s], f);
        if (nb > max_blocks)
            max_blocks = nb;
    }
    const hipError_t e = launch_spec(a, max_blocks, b->stream);
    if (e != hipSuccess)
        return fail(COOLMIC_ERROR_GENERIC, "run: the spectrum pass: %s", hipGetErrorString(e));
    g_spec_runs.fetch_add(1, std::memory_order_relaxed);
    b->spec_parity ^= 1u;                    // the kernel wrote the other state slot
    for (unsigned s = 0; s < b->d.streams; s++) {
        const uint32_t f = frames_per_stream ? frames_per_stream[s] : (uint32_t)frames;
        b->spec_blocks[s] += spec_run_blocks(b->spec_log2, b->spec_back[s], f);
        b->spec_back[s] = spec_next_back(b->spec_log2, b->spec_back[s], f);
    }
    b->spec.account(frames, frames_per_stream);
    return COOLMIC_ERROR_NONE;
}

// one window's result from its sums; out is left alone while the window holds no block
static int spec_finish(const cmhip_batch_t *b, size_t s, const void *window, const void *, void *result)
{
    const unsigned long long blocks = b->spec_blocks[s];
    if (blocks == 0)
        return COOLMIC_ERROR_INVAL;
    const unsigned long long *const sums = (const unsigned long long *)window;
    coolmic_spectrum_result_t *const out = (coolmic_spectrum_result_t *)result;
    memset(out, 0, sizeof(*out));
    out->rate = b->d.rate;
    out->channels = b->d.channels;
    out->frames = (size_t)b->spec.frames[s];
    out->blocks = (size_t)blocks;
    out->fft_log2 = b->spec_log2;
    out->bands = b->spec_nb;
    out->selected = b->spec_nch;
    memcpy(out->edges, b->spec_edges, (b->spec_nb + 1) * sizeof(uint16_t));
    memcpy(out->channel, b->spec_ch, b->spec_nch);
    for (unsigned c = 0; c < b->spec_nch; c++)
        for (unsigned k = 0; k < b->spec_nb; k++) {
            out->power[c][k] = sums[c * SPEC_MAX_BANDS + k];
            out->db[c][k] = spec_db(out->power[c][k], blocks);
        }
    return COOLMIC_ERROR_NONE;
}

static const MeterKind SPEC = {"spec", "spectrum", "the spectrum", &cmhip_batch::spec, sizeof(coolmic_spectrum_result_t),
                               spec_finish, spec_turn_on};

extern "C" int cmhip_batch_set_spectrum(cmhip_batch_t *b, int on)
{
    return cmhip_meter_switch(b, SPEC, on);  // (the geometry stays across off and on)
}

extern "C" int cmhip_batch_get_spectrum(const cmhip_batch_t *b) { return cmhip_meter_get(b, SPEC); }

// A window closes on its blocks, not its frames: frames short of a block give no result and are kept.
extern "C" int cmhip_batch_spec_result(cmhip_batch_t *b, unsigned int stream, coolmic_spectrum_result_t *out)
{
    if (b && out && b->spec.on && stream < b->d.streams && b->spec_blocks[stream] == 0)
        return fail(COOLMIC_ERROR_INVAL, "spec_result: the window holds no completed block");
    const int rc = cmhip_meter_fetch_one(b, SPEC, stream, out);
    if (rc == COOLMIC_ERROR_NONE)
        b->spec_blocks[stream] = 0;
    return rc;
}

extern "C" int cmhip_batch_spec_results(cmhip_batch_t *b, coolmic_spectrum_result_t *out, int *rc)
{
    const int r = cmhip_meter_fetch_all(b, SPEC, out, rc);
    // every window that held a block has closed, frames and all; the others keep their frames and had no block
    if (r == COOLMIC_ERROR_NONE)
        b->spec_blocks.assign(b->d.streams, 0);
    return r;
}

extern "C" int cmhip_batch_spec_reset(cmhip_batch_t *b, long stream)
{
    size_t lo, n;
    const int rc = cmhip_meter_clear_range(b, SPEC, stream, &lo, &n);
    if (rc != COOLMIC_ERROR_NONE)
        return rc;
    const size_t S = b->d.streams;
    const size_t row = (size_t)b->spec_nch << b->spec_log2;      // state samples per stream and slot
    for (size_t slot = 0; slot < 2; slot++) {
        HIP_TRY(hipMemsetAsync(b->d_spec_hist + (slot * S + lo) * row, 0, n * row * sizeof(int16_t), b->stream));
        HIP_TRY(hipMemsetAsync(b->d_spec_back + slot * S + lo, 0, n * sizeof(uint32_t), b->stream));
    }
    for (size_t s = lo; s < lo + n; s++) {
        b->spec_back[s] = 0;
        b->spec_blocks[s] = 0;
    }
    return COOLMIC_ERROR_NONE;
}
