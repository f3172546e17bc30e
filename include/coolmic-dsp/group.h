/*
 * group.h -- many transform -> vumeter pipelines served by ONE launch per block.
 *
 * Not in the reference.  A host that runs thousands of capture streams builds one
 * coolmic_group_t instead of thousands of coolmic_transform_t / coolmic_vumeter_t
 * pairs; every stream keeps the reference's operator interface on both sides:
 *
 *   upstream:    any coolmic_iohandle_t per stream (snddev, file, user callback)
 *   downstream:  coolmic_group_get_iohandle(slot) -- a coolmic_iohandle_t that delivers
 *                the stream's transformed PCM in whole frames, like the handle of
 *                coolmic_transform_get_iohandle() (ref: src/transform.c:126-193)
 *   meter:       coolmic_group_vumeter_result(slot) -- the contract of
 *                coolmic_vumeter_result() (ref: src/vumeter.c:189-218)
 *
 * coolmic_group_pump() moves one block: it pulls up to block_frames from every
 * upstream handle into pinned staging (partial frames are carried to the next pump,
 * as ref: src/transform.c:155-160 does per read) and queues upload, the fused
 * channel-map/gain/VU kernel over all streams and the download on the GPU -- then it
 * returns.  The block's PCM reaches the streams' output queues with the next pump or
 * with the first read that finds a queue empty, so a host that pumps and reads in a
 * loop reads block k while the GPU works on block k+1.  A read on an empty downstream
 * handle first brings the block in flight home and only then pumps by itself, so a
 * purely pull-driven chain works unchanged and never pulls more than it did; streams
 * are read ahead by at most `queue_blocks` blocks (the block in flight counts; use
 * >= 2 for the overlap), and parameter changes take effect at the next pump.
 */
#ifndef __COOLMIC_DSP_GROUP_H__
#define __COOLMIC_DSP_GROUP_H__

#include <stdint.h>
#include <sys/types.h>
#include "ro-compat.h"
#include "iohandle.h"
#include "vumeter.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct coolmic_group coolmic_group_t;

/* NULL for rate/channels/max_streams/block_frames of 0, channels > 16, or no usable GPU.
 * queue_blocks >= 1 is how many processed blocks a stream may hold unread. */
coolmic_group_t    *coolmic_group_new(const char *name, igloo_ro_t associated, uint_least32_t rate,
                                      unsigned int channels, unsigned int max_streams,
                                      size_t block_frames, unsigned int queue_blocks);

/* The same group on a GPU of the caller's choice instead of $COOLMIC_HIP_DEVICE (default 0): a host that drives
 * every GPU of a node from one process makes one group per GPU and gives capture stream s to the group of GPU
 * s % N, one pump thread per group (examples/group_server.c --gpus N).  NULL also for a device the
 * process does not see. */
coolmic_group_t    *coolmic_group_new_on(int device, const char *name, igloo_ro_t associated, uint_least32_t rate,
                                         unsigned int channels, unsigned int max_streams,
                                         size_t block_frames, unsigned int queue_blocks);
/* the GPU a group lives on; -1 for NULL */
int                 coolmic_group_device(coolmic_group_t *self);
/* the group's batch engine (cmhip_batch_t of <coolmic_hip.h>), for what the group itself does not wrap: the
 * node-global VU over the groups of several GPUs (cmhip_node_partial(node, engine, ...) after a pump; the record
 * counts the block that pump put in flight).  Owned by the group; not to be run, resized or freed. */
struct cmhip_batch *coolmic_group_engine(coolmic_group_t *self);

/* adds a stream fed by `source` (takes its own reference); returns the slot (>= 0) or
 * COOLMIC_ERROR_FAULT / COOLMIC_ERROR_BUSY when the group is full */
int                 coolmic_group_add_stream(coolmic_group_t *self, coolmic_iohandle_t *source);

/* per-stream parameters, rules of coolmic_transform_set_master_gain / _set_channel_map */
int                 coolmic_group_set_master_gain(coolmic_group_t *self, unsigned int slot,
                                                  unsigned int channels, uint16_t scale,
                                                  const uint16_t *gain);
int                 coolmic_group_set_channel_map(coolmic_group_t *self, unsigned int slot,
                                                  const uint8_t *map);
/* equaliser as coolmic_transform_set_eq().  The number of sections is one for the whole
 * group: slot -1 sets every stream (and may change the count), a slot >= 0 only replaces
 * that stream's coefficients and must keep the count (else COOLMIC_ERROR_INVAL). */
int                 coolmic_group_set_eq(coolmic_group_t *self, int slot, unsigned int sections,
                                         const float *coef);

/* transformed PCM of one stream; keeps the group alive while it lives */
coolmic_iohandle_t *coolmic_group_get_iohandle(coolmic_group_t *self, unsigned int slot);

/* one block for every stream whose queue has room.  Returns the number of streams whose source
 * delivered at least one frame to this block, 0 when no source had anything (the block that was
 * in flight is in the queues then), negative on error. */
int                 coolmic_group_pump(coolmic_group_t *self);

/* The pull of a pump -- one read per upstream handle -- spread over `threads` threads (the pumping thread
 * counts; 0 or 1: the pumping thread alone, which is how a group starts).  The handles of DIFFERENT streams
 * are then read at the same time, each stream's own handle still by one thread at a time and once per pump:
 * fine for the sources of this library and for callbacks that keep their state per stream, as the reference's
 * pipelines do with one thread each (ref: src/simple.c:292-310).
 * Streams that read from one object stay on the pumping thread, in slot order, after the other threads have
 * finished.  Recognised, when a stream is added, are: the same handle given twice; handles with the same
 * userdata (two handles of one sound device); the reader handles of one coolmic_tee_t; and any of these behind
 * chains of this library's transforms and tees (two transforms fed by two readers of one tee, or both fed by
 * one device handle; a tee whose input is a reader of another tee), followed through the inputs that are
 * attached at that moment -- a chain of 64 wrappers or more is not followed to its end and keeps its stream
 * on the pumping thread whatever it shares.
 * NOT recognised, and the caller's to keep thread-safe or off one group: read callbacks of different userdata
 * that share state behind it; and whatever is attached or re-attached (coolmic_tee_attach_iohandle,
 * coolmic_transform_attach_iohandle) upstream of a stream's handle after coolmic_group_add_stream -- attach
 * first, add the stream afterwards.  COOLMIC_ERROR_INVAL for more than 64 threads. */
int                 coolmic_group_set_pull_threads(coolmic_group_t *self, unsigned int threads);

/* VU window of one stream since its last result; COOLMIC_ERROR_INVAL while it holds no frame */
int                 coolmic_group_vumeter_result(coolmic_group_t *self, unsigned int slot,
                                                 coolmic_vumeter_result_t *result);

/* Every stream's VU window since its last result, all closed at one point -- after everything pumped so far, the
 * block in flight included -- in ONE snapshot and collect of the group's engine instead of a copy and a wait per
 * stream.  results[] and rc[] (rc may be NULL) have coolmic_group_streams() entries; per slot the contract of
 * coolmic_group_vumeter_result(): rc[slot] is COOLMIC_ERROR_INVAL and results[slot] is left alone for a window
 * without a frame. */
int                 coolmic_group_vumeter_results(coolmic_group_t *self, coolmic_vumeter_result_t *results, int *rc);

/* Where coolmic_group_vumeter_results() finishes the dB values: CMHIP_VU_FINISH_HOST (0, how a group starts:
 * bit-equal to coolmic_vumeter_result()) or CMHIP_VU_FINISH_DEVICE (1: no host arithmetic, last bits of the power
 * doubles may differ) of <coolmic_hip.h>, with cmhip_batch_vu_set_finish()'s return values.
 * coolmic_group_vumeter_result() for one slot is finished on the host either way. */
int                 coolmic_group_set_vu_finish(coolmic_group_t *self, int where);

/* True peak (ITU-R BS.1770 Annex 2, 4x oversampling) of every stream, opt-in: cmhip_batch_set_true_peak() of
 * <coolmic_hip.h> on the group's engine, with its return values.  While it is on every block runs the true-peak
 * kernel ahead of the block kernel; the group's blocks lie in host memory, so the input set is read a SECOND time
 * over PCIe -- that read is the cost of the group form.  The filter measures the transformed stream (map, gain,
 * saturation), not the equaliser's result: coolmic_group_set_eq() with sections returns COOLMIC_ERROR_INVAL while
 * true peak is on, and turning it on does while the group's equaliser has sections. */
int                 coolmic_group_set_true_peak(coolmic_group_t *self, int on);
/* One slot's true-peak window since its last result, and all of them at once (results[] and rc[], which may be
 * NULL, have coolmic_group_streams() entries): the slot handling and the per-slot contract of
 * coolmic_group_vumeter_result(s) -- COOLMIC_ERROR_INVAL with the result left alone for a window without a frame,
 * the window closed after everything pumped so far, the block in flight included.  The true-peak windows are
 * independent of the VU windows; a host that wants them aligned asks for both between the same two pumps. */
int                 coolmic_group_true_peak(coolmic_group_t *self, unsigned int slot, coolmic_truepeak_result_t *result);
int                 coolmic_group_true_peaks(coolmic_group_t *self, coolmic_truepeak_result_t *results, int *rc);

/* Programme loudness (ITU-R BS.1770 / EBU R128) of every stream, opt-in: cmhip_batch_set_loudness() of
 * <coolmic_hip.h> on the group's engine, with its return values and its specification.  While it is on every block
 * runs the loudness kernel ahead of the block kernel (beside the true-peak kernel when that is on too); the group's
 * blocks lie in host memory, so the input set is read once more over PCIe.  It measures the transformed stream, not
 * the equaliser's result: the two exclude each other with COOLMIC_ERROR_INVAL both ways round. */
int                 coolmic_group_set_loudness(coolmic_group_t *self, int on);
/* One slot's loudness since the group turned it on or the slot was reset, and all of them at once (results[] and
 * rc[], which may be NULL, have coolmic_group_streams() entries): the slot handling of coolmic_group_true_peak(s).
 * NOT destructive -- loudness integrates until coolmic_group_loudness_reset (slot -1: all).  rc[] is
 * COOLMIC_ERROR_NONE for every slot: a slot without a frame reports zeros and -inf.  Everything pumped so far
 * counts, the block in flight included. */
int                 coolmic_group_loudness(coolmic_group_t *self, unsigned int slot, coolmic_loudness_result_t *result);
int                 coolmic_group_loudnesses(coolmic_group_t *self, coolmic_loudness_result_t *results, int *rc);
/* cmhip_batch_loud_set_weights / cmhip_batch_loud_reset for a slot, or -1 for every stream of the engine */
int                 coolmic_group_loudness_set_weights(coolmic_group_t *self, long slot, const double *weights);
int                 coolmic_group_loudness_reset(coolmic_group_t *self, long slot);

/* Phase correlation and balance of every stream's channel pairs, opt-in: cmhip_batch_set_correlation() of
 * <coolmic_hip.h> on the group's engine, with its return values and its specification (a mono group cannot be
 * metered).  While it is on every block runs the correlation kernel ahead of the block kernel (beside the true-peak
 * and loudness kernels when those are on too); the group's blocks lie in host memory, so the input set is read once
 * more over PCIe -- that read is the cost of the group form.  It measures the transformed stream, not the
 * equaliser's result: the two exclude each other with COOLMIC_ERROR_INVAL both ways round. */
int                 coolmic_group_set_correlation(coolmic_group_t *self, int on);
/* cmhip_batch_corr_set_pairs for the group's engine: the pairs are the same for every slot, and change only while
 * every window is empty (COOLMIC_ERROR_BUSY otherwise). */
int                 coolmic_group_correlation_set_pairs(coolmic_group_t *self, unsigned int n, const unsigned char pairs[][2]);
/* One slot's correlation window since its last result, and all of them at once (results[] and rc[], which may be
 * NULL, have coolmic_group_streams() entries): the slot handling and the per-slot contract of
 * coolmic_group_true_peak(s) -- COOLMIC_ERROR_INVAL with the result left alone for a window without a frame, the
 * window closed after everything pumped so far, the block in flight included.  coolmic_group_correlation_reset
 * clears a slot's window, or with -1 every window of the engine. */
int                 coolmic_group_correlation(coolmic_group_t *self, unsigned int slot, coolmic_correlation_result_t *result);
int                 coolmic_group_correlations(coolmic_group_t *self, coolmic_correlation_result_t *results, int *rc);
int                 coolmic_group_correlation_reset(coolmic_group_t *self, long slot);

/* The spectrum of every stream's selected channels, opt-in: cmhip_batch_set_spectrum() of <coolmic_hip.h> on the
 * group's engine, with its return values and its specification (mono groups included).  While it is on every block
 * runs the spectrum kernel ahead of the block kernel, beside the other meters' kernels; as with correlation the input
 * set is read once more over PCIe.  It measures the transformed stream, not the equaliser's result: the two exclude
 * each other with COOLMIC_ERROR_INVAL both ways round. */
int                 coolmic_group_set_spectrum(coolmic_group_t *self, int on);
/* cmhip_batch_spec_configure for the group's engine: block size, band table and channels are the same for every
 * slot, and change only while the meter is off (COOLMIC_ERROR_BUSY otherwise). */
int                 coolmic_group_spectrum_configure(coolmic_group_t *self, unsigned int fft_log2, unsigned int nb,
                                                     const uint16_t *edges, unsigned int nch, const unsigned char *channels);
/* One slot's spectrum window since its last result, and all of them at once (results[] and rc[], which may be NULL,
 * have coolmic_group_streams() entries): the slot handling of coolmic_group_correlation(s) --
 * COOLMIC_ERROR_INVAL with the result left alone and the window kept for a window without a completed block.
 * coolmic_group_spectrum_reset clears a slot's window, state and position, or with -1 those of every slot. */
int                 coolmic_group_spectrum(coolmic_group_t *self, unsigned int slot, coolmic_spectrum_result_t *result);
int                 coolmic_group_spectra(coolmic_group_t *self, coolmic_spectrum_result_t *results, int *rc);
int                 coolmic_group_spectrum_reset(coolmic_group_t *self, long slot);

/* The signal watch -- dead air, clipping, DC offset of every stream -- opt-in: cmhip_batch_set_watch() of
 * <coolmic_hip.h> on the group's engine, with its return values and its specification (mono groups included).  While
 * it is on every block runs the watch's two kernels ahead of the block kernel, beside the other meters' kernels; as
 * with correlation the input set is read once more over PCIe.  Run lengths continue from block to block and from
 * window to window.  It measures the transformed stream, not the equaliser's result: the two exclude each other with
 * COOLMIC_ERROR_INVAL both ways round. */
int                 coolmic_group_set_watch(coolmic_group_t *self, int on);
/* cmhip_batch_watch_configure for the group's engine: the thresholds are the same for every slot, and change only
 * while every window is empty (COOLMIC_ERROR_BUSY otherwise); a change clears every slot's run state. */
int                 coolmic_group_watch_configure(coolmic_group_t *self, unsigned int quiet, unsigned int rail,
                                                  unsigned int clip_run);
/* One slot's watch window since its last result, and all of them at once (results[] and rc[], which may be NULL, have
 * coolmic_group_streams() entries): the slot handling of coolmic_group_correlation(s) -- COOLMIC_ERROR_INVAL with the
 * result left alone for a window without a frame.  A result closes the window and keeps the run state;
 * coolmic_group_watch_reset clears a slot's window and state, or with -1 those of every slot. */
int                 coolmic_group_watch(coolmic_group_t *self, unsigned int slot, coolmic_watch_result_t *result);
int                 coolmic_group_watches(coolmic_group_t *self, coolmic_watch_result_t *results, int *rc);
int                 coolmic_group_watch_reset(coolmic_group_t *self, long slot);

unsigned int        coolmic_group_streams(coolmic_group_t *self);

#ifdef __cplusplus
}
#endif
#endif
