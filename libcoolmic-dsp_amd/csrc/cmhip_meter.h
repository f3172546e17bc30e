// cmhip_meter.h -- what the batch's window meters (true peak, correlation, spectrum, watch) share on the host: the
// state of one meter's windows and the lifecycle around it -- the switch, the frames a run adds, one window's or all
// windows' results, the reset.  A meter's file supplies its MeterKind (names, result size, finish, what else turning
// it on makes and clears), its kernel's launch and whatever state it keeps beside the windows; the functions are
// defined in cmhip_batch.hip.  Loudness has a ring, not a window (cmhip_loud.hip), and uses none of this.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <vector>

struct cmhip_batch;

struct CMHIP_INTERNAL WindowMeter {
    explicit WindowMeter(size_t bytes, size_t state_bytes = 0) : bytes(bytes), state_bytes(state_bytes) {}

    bool on = false;
    void *d = nullptr;                         // [S][bytes] the windows and behind them [S][state_bytes] the state
    const size_t bytes;                        // per stream of window: what a result reads and clears
    const size_t state_bytes;                  // per stream of state that results keep and on / reset clear (the watch)
    std::vector<unsigned long long> frames;    // frames accounted per stream since its window opened
    std::vector<unsigned long long> host;      // staging of a results call: all windows, then all state (8-byte words)

    template <class T> T *windows() const { return (T *)d; }
    template <class T> T *state(size_t streams) const { return (T *)((unsigned char *)d + streams * bytes); }

    // the frames of a run that has been queued (frames_per_stream: the run's host array or nullptr)
    void account(size_t run_frames, const uint32_t *frames_per_stream)
    {
        for (size_t s = 0; s < frames.size(); s++)
            frames[s] += frames_per_stream ? frames_per_stream[s] : run_frames;
    }

    bool windows_empty() const
    {
        if (!on)
            return true;
        for (unsigned long long f : frames)
            if (f)
                return false;
        return true;
    }
};

struct MeterKind {
    const char *tag;                           // "tp": the calls' names in messages are tp_result, tp_results, tp_reset
    const char *sw;                            // "true_peak": ... and set_true_peak, get_true_peak
    const char *name;                          // "true peak": the meter in a sentence
    WindowMeter cmhip_batch::*meter;
    size_t out_size;                           // of the meter's result struct
    // stream s's result from its staged window (and state); COOLMIC_ERROR_INVAL and `out` left alone while the window
    // holds nothing to close
    int (*finish)(const cmhip_batch *b, size_t s, const void *window, const void *state, void *out);
    // turning the meter on: what it makes and clears beside the windows, or nullptr -> an error number
    int (*turn_on)(cmhip_batch *b);
};

// set_X after the meter's own precondition: NULL, the equaliser's sections, use, the stream's end, off, already on;
// then turn_on, the windows (made once), their clearing, the counts
CMHIP_INTERNAL int cmhip_meter_switch(cmhip_batch *b, const MeterKind &k, int on);
CMHIP_INTERNAL int cmhip_meter_get(const cmhip_batch *b, const MeterKind &k);
// X_result: one window copied, finished, cleared on the stream (the state stays), its count zeroed
CMHIP_INTERNAL int cmhip_meter_fetch_one(cmhip_batch *b, const MeterKind &k, unsigned int stream, void *out);
// X_results: one round trip for all streams; rc[s] is the finish's word, and a window it refused keeps its count
CMHIP_INTERNAL int cmhip_meter_fetch_all(cmhip_batch *b, const MeterKind &k, void *out, int *rc);
// X_reset: windows, state and counts of stream `stream` (-1: all) cleared; lo / n, where asked for: the range, for
// what the meter keeps beside them
CMHIP_INTERNAL int cmhip_meter_clear_range(cmhip_batch *b, const MeterKind &k, long stream, size_t *lo = nullptr,
                                           size_t *n = nullptr);
