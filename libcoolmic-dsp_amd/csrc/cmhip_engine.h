// cmhip_engine.h -- the batch object and what the engine's translation units share (not part of the C ABI):
//   cmhip_batch.hip    the object, parameters, transfers, the run, the list of meters and the window meters' shared
//                      lifecycle (csrc/cmhip_meter.h)
//   cmhip_place.hip    the opt-in placement search for a batch's two PCM arrays
//   cmhip_vu.hip       VU windows: results, packed snapshots and their collect, window records, node records
//   cmhip_tp.hip       true peak: its kind and history, its launch ahead of a run, the finish
//   cmhip_corr.hip     phase correlation: its kind and pairs, its launch ahead of a run, the finish
//   cmhip_spec.hip     spectrum: its kind, geometry and state, its launch ahead of a run, the finish
//   cmhip_watch.hip    signal watch: its kind and thresholds, its launch ahead of a run, the finish
//   cmhip_loud.hip     loudness: the opt-in state, its launch ahead of a run, the ring's drain, results
//   cmhip_measure.hip  kernel timing and the plain HBM ceilings
//   node.hip           the node-global VU exchange over RCCL (cmhip_node_*)
// and the stage objects beside the batch, which use fail, HIP_TRY and csrc/cmhip_stage.h only:
//   cmhip_src.hip      sample-rate conversion
//   cmhip_mix.hip      channel mixing and matrix ramps
//   cmhip_bus.hip      the mix bus
//   cmhip_lim.hip      the peak limiter
//   cmhip_dyn.hip      the dynamics stage: compressor and gate
//   cmhip_split.hip    the band split: an FIR crossover
//   cmhip_delay.hip    the delay line
//   cmhip_agc.hip      the leveller: slow automatic gain control
//   cmhip_automix.hip  the automixer: gain-sharing groups
//   cmhip_failover.hip the failover switch: silence-triggered source changeover
//   cmhip_drift.hip    the drift stage: a variable-ratio resampler against clock drift
//   cmhip_iir.hip      the filter: a biquad cascade in exact integers
//   cmhip_denoise.hip  the noise suppressor: a spectral gate in exact integers
#pragma once

#include "cmhip_internal.h"

#include <coolmic-dsp/coolmic-dsp.h>
#include <coolmic_hip.h>

#include <vector>

#include "work_pool.h"
#include "host_internal.h"

using namespace cmhip;

#define CMHIP_INTERNAL __attribute__((visibility("hidden")))
CMHIP_INTERNAL int cmhip_fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
#define fail cmhip_fail

#define HIP_TRY(expr)                                                                       \
    do {                                                                                    \
        hipError_t e_ = (expr);                                                             \
        if (e_ != hipSuccess)                                                               \
            return fail(COOLMIC_ERROR_GENERIC, "%s: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                        __FILE__, __LINE__);                                                \
    } while (0)

#include "cmhip_stage.h"
#include "cmhip_meter.h"

constexpr unsigned STAGE_SLOTS = 4;
constexpr size_t STAGE_BYTES = 64 * 1024;

struct EventPair {
    hipEvent_t a, b;
};

struct cmhip_batch {
    cmhip_batch_desc_t d;
    hipStream_t stream;
    bool own_stream;
    size_t stride;                 // samples between slots
    size_t plane;                  // floats between f32 planes

    int16_t *d_in, *d_out;
    int16_t *h_in, *h_out;         // CMHIP_HOSTPCM: the slots live in pinned host memory (d_* alias them)
    bool in_flight;                // a launch may still be using the slots (CMHIP_HOSTPCM)
    // CMHIP_HOSTPCM: a launch of one workgroup reports its end through a word in pinned, device-mapped host
    // memory (RunArgs::done_flag) and the host spins on it -- 4-5 us less per pull than waiting for the stream
    uint32_t *h_done, *d_done;
    uint32_t done_seq;             // the last sequence number handed to a launch
    bool done_flagged;             // ... and that launch carries the flag
    float *d_f32;
    StreamParam *d_param;
    VuState *d_vu;                         // the window runs accumulate into (= d_vu2[cur])
    VuState *d_vu2[3];                     // three sets in rotation: accumulating / being copied out / cleared
    unsigned int cur;
    hipStream_t copy_stream;               // snapshots travel here, beside the next run
    hipEvent_t ev_main, ev_reset[3];
    // A node partial (cmhip_node_partial) reads the current windows on the copy stream, beside the next
    // run; node_reading is set until the window set has rotated (snapshot) or the main stream has been
    // made to wait for the copy stream (settle_node: before anything on the main stream touches them).
    hipEvent_t ev_node;
    bool node_reading;
    // The end of the last run as its own dispatch stamped it (hipExtLaunchKernelGGL): what a snapshot
    // makes the copy stream wait for instead of an event recorded behind the kernel -- one packet less
    // on the main stream per step.  nullptr once anything else on the main stream touched the windows.
    hipEvent_t ev_done[4], last_done;
    unsigned done_next;
    bool reset_pending[3];
    struct WorkPool *pool;
    uint32_t *d_nframes;
    CountsRing counts;                 // a run's counts on their way to d_nframes
    EqParam *d_eq;
    EqState *d_eqstate;
    unsigned long long *d_sink;
    long long *d_node_scratch;             // one node record, for cmhip_batch_vu_node_record (made on first use)
    // ring mode (cmhip_batch_vu_ring): every run accumulates into a window of its own
    VuState *d_ring, *h_ring;              // ring_slots x S windows on the device / pinned staging for a fetch
    unsigned int ring_slots;
    uint64_t ring_seq;                     // sequence number of the next run
    uint64_t ring_fetched;                 // runs below this sequence number have been fetched: their slots are clear

    std::vector<StreamParam> h_param;
    std::vector<uint16_t> h_scale;         // the reference's master_gain_scale per stream
    std::vector<uint16_t> h_gain;          // [S][16]
    bool param_dirty = true;
    bool all_identity = true;              // no stream has a channel map (recomputed on upload)
    std::vector<EqParam> h_eq;
    unsigned int nsec;
    bool eq_dirty;

    // three snapshots may be pending (one being finished by the helper threads, one waiting, one on its way):
    // each a packed copy of a window set, [1 + 2C][S] words in pinned, device-mapped host memory that
    // k_vu_pack writes itself (h_pack / d_pack: host / device view).  With vu_finish == CMHIP_VU_FINISH_DEVICE
    // k_vu_finish writes finished records there instead (never longer); the mode changes only while no snapshot
    // is pending, so a slot is always read the way it was written.
    unsigned long long *h_pack[3], *d_pack[3];
    int vu_finish = CMHIP_VU_FINISH_HOST;  // cmhip_batch_vu_set_finish
    unsigned int snap_set2[3];             // which of the three window sets the snapshot closed (its event: ev_reset)
    bool collecting;                       // between cmhip_batch_vu_collect_begin and _end
    coolmic_vumeter_result_t *job_out;
    int *job_rc;
    unsigned int job_slot;
    unsigned int snap_head, snap_count;    // ring of pending snapshots (oldest = head)
    unsigned char *h_stage;                // pinned upload ring, STAGE_SLOTS x STAGE_BYTES
    hipEvent_t stage_ev[4];
    bool stage_busy[4];
    unsigned int stage_next;
    unsigned int parity;                   // current slot of VuState::samples

    bool timing;
    unsigned int timing_every = 1, timing_count;  // every n-th run carries the events (cmhip_batch_timing)
    std::vector<EventPair> ev_used, ev_free;
    // what the placement search did (cmhip_batch_placement); without one, candidates 0 and 1 -- the arrays where
    // hipMalloc put them -- are the input and the output
    cmhip_placement_t place = {0, 2, 0, 1, 0, 0, 0, 0, 0, 0};
    bool vu_off;                           // runs leave the windows alone for now (cmhip_batch_vu_pause)

    // The window meters (csrc/cmhip_meter.h), each with what it keeps beside its windows.
    // true peak (cmhip_tp.hip), all of it unused until cmhip_batch_set_true_peak(b, 1)
    WindowMeter tp{MAX_CH * sizeof(uint32_t)};             // [S][16] window maxima of |y|
    int16_t *d_tp_hist = nullptr;          // [2][S][16][11] the streams' filter history, slot tp_parity current
    unsigned int tp_parity = 0;
    // phase correlation (cmhip_corr.hip), all of it but the pairs unused until cmhip_batch_set_correlation(b, 1)
    WindowMeter corr{CORR_MAX_PAIRS * CORR_SUMS * sizeof(unsigned long long)};     // [S][8][3] energy_a, energy_b, cross
    unsigned int corr_npairs = 1;          // the channel pairs, the same for all streams (kept across off / on)
    unsigned char corr_a[CORR_MAX_PAIRS] = {0}, corr_b[CORR_MAX_PAIRS] = {1};
    // spectrum (cmhip_spec.hip), all of it but the geometry unused until cmhip_batch_set_spectrum(b, 1)
    WindowMeter spec{SPEC_MAX_CH * SPEC_MAX_BANDS * sizeof(unsigned long long)};   // [S][8][32] sums per selected channel and band
    int16_t *d_spec_hist = nullptr;        // [2][S][nch][N] the streams' last N - 1 samples, slot spec_parity current
    uint32_t *d_spec_back = nullptr;       // [2][S] the streams' back (csrc/spec_plan.h), slot spec_parity current
    int32_t *d_spec_table = nullptr;       // Wr[N/2], Wi[N/2], win[N], edges[33]
    size_t spec_hist_words = 0, spec_table_words = 0;   // what the two arrays were allocated for
    unsigned int spec_parity = 0;
    // the geometry, the same for all streams (kept across off / on); spec_nb 0 / spec_nch 0: the defaults, filled in
    // when the meter is turned on
    unsigned int spec_log2 = SPEC_DEFAULT_LOG2;
    unsigned int spec_nb = 0, spec_nch = 0;
    uint16_t spec_edges[SPEC_MAX_BANDS + 1] = {};
    unsigned char spec_ch[SPEC_MAX_CH] = {};
    std::vector<uint32_t> spec_back;             // host mirror of the current back per stream
    std::vector<unsigned long long> spec_blocks; // blocks summed per stream since its window opened
    // signal watch (cmhip_watch.hip), all of it but the thresholds unused until cmhip_batch_set_watch(b, 1)
    WindowMeter watch{WATCH_WINDOW_WORDS * sizeof(unsigned long long), WATCH_SLOTS * sizeof(unsigned long long)};
    WatchSum *d_watch_scratch = nullptr;   // [S][tiles][2C + 1] a run's tile summaries, grown on need
    uint64_t watch_scratch_n = 0;          // summaries d_watch_scratch holds
    unsigned int watch_quiet = WATCH_DEFAULT_QUIET, watch_rail = WATCH_DEFAULT_RAIL, watch_run = WATCH_DEFAULT_RUN;
    // loudness (cmhip_loud.hip), all of it unused until cmhip_batch_set_loudness(b, 1)
    bool loud_on = false;
    LoudState *d_loud = nullptr;           // [S][C] the rows' filter history and open sub-block
    double *d_loud_ring = nullptr;         // [S][loud_slots][C] completed sub-block sums
    unsigned int loud_sub = 0;             // L: frames per sub-block
    unsigned int loud_slots = 0;           // R: sub-blocks the ring holds per stream
    double loud_coef[10] = {};
    std::vector<double> loud_w;            // [S][C] channel weights (kept across enable / reset)
    std::vector<unsigned long long> loud_frames;    // frames per stream since enable / reset: completed = frames / L
    std::vector<unsigned long long> loud_drained;   // sub-blocks per stream taken out of the ring so far
    std::vector<std::vector<double>> loud_z;        // per stream: z_j of every drained sub-block
    std::vector<double> loud_recent;       // [S][30][C] per-channel sums of the trailing sub-blocks, number j at j % 30
    std::vector<double> loud_host;         // [S][loud_slots][C] staging of a drain
};


static inline int use(cmhip_batch_t *b)
{
    HIP_TRY(hipSetDevice(b->d.device));
    return COOLMIC_ERROR_NONE;
}

// the main stream is about to touch the windows a node partial may still be reading on the copy stream
CMHIP_INTERNAL int cmhip_engine_settle_node(cmhip_batch_t *b);
// parameter and equaliser tables to the device, when a setter has run since the last upload
CMHIP_INTERNAL int cmhip_engine_flush_params(cmhip_batch_t *b);
// the RunArgs of a run of this batch (nframes: per-stream frame counts on the device, or nullptr; window: the VU
// windows, or nullptr); the completion flag is left to the caller
CMHIP_INTERNAL RunArgs cmhip_engine_run_args(const cmhip_batch_t *b, const int16_t *in, int16_t *out, size_t frames,
                                             const uint32_t *nframes, VuState *window, uint32_t parity);
// cmhip_tp.hip: the true-peak pass of a run over `in`, queued on the batch's stream ahead of the block kernel
// (only called while b->tp.on; frames_per_stream: the run's host array or nullptr, already uploaded to d_nframes)
CMHIP_INTERNAL int cmhip_engine_tp_run(cmhip_batch_t *b, const int16_t *in, size_t frames,
                                       const uint32_t *frames_per_stream);
// cmhip_corr.hip: the correlation pass of a run over `in`, queued on the batch's stream ahead of the block kernel
// (only called while b->corr.on; frames_per_stream as for cmhip_engine_tp_run)
CMHIP_INTERNAL int cmhip_engine_corr_run(cmhip_batch_t *b, const int16_t *in, size_t frames,
                                         const uint32_t *frames_per_stream);
// cmhip_spec.hip: the spectrum pass of a run over `in`, queued on the batch's stream ahead of the block kernel
// (only called while b->spec.on; frames_per_stream as for cmhip_engine_tp_run)
CMHIP_INTERNAL int cmhip_engine_spec_run(cmhip_batch_t *b, const int16_t *in, size_t frames,
                                         const uint32_t *frames_per_stream);
// cmhip_watch.hip: the watch's tile pass and fold of a run over `in`, queued on the batch's stream ahead of the block
// kernel (only called while b->watch.on; frames_per_stream as for cmhip_engine_tp_run)
CMHIP_INTERNAL int cmhip_engine_watch_run(cmhip_batch_t *b, const int16_t *in, size_t frames,
                                          const uint32_t *frames_per_stream);
// cmhip_loud.hip: the loudness pass of a run over `in`, queued on the batch's stream ahead of the block kernel (only
// called while b->loud_on; drains the ring first when the run could overflow it).  Returns an error number.
CMHIP_INTERNAL int cmhip_engine_loud_run(cmhip_batch_t *b, const int16_t *in, size_t frames,
                                         const uint32_t *frames_per_stream);
// cmhip_place.hip: called once, at the end of a batch's creation, when it has PCM arrays of its own
CMHIP_INTERNAL int cmhip_engine_place_arrays_apart(cmhip_batch_t *b, size_t bytes);
// cmhip_vu.hip (for node.hip): the node record of the batch's windows, built on the copy stream
CMHIP_INTERNAL int cmhip_batch_node_partial_side(cmhip_batch_t *b, long long *dst_sum, long long *dst_key,
                                                 uint64_t first_global, uint64_t global_step);
