// pipe_internal.h -- the packet pipeline's handle, shared by pipe.hip (one batch) and rt.hip (the real-time tick over several batches).
#pragma once
#include <vector>
#include "slot_ring.h"

namespace wmx {
constexpr int kDatagram = 172;  // 12-byte RTP header + 160 G.711 codes (20 ms at 8 kHz), src/rtp.h:33, src/rtp.c:86-95
constexpr int kPipeFreq = 8000, kPkt10 = 80;
}  // namespace wmx

struct wmx_pipe {
    int device;  // first member of every handle (wmx_handle_device)
    int n_streams;
    bool pcm;          // rows are PCM packages (wmx_pipe_create_pcm), not RTP datagrams
    bool far_rows;     // every stream hears a far-end of its own (wmx_pipe_create_pcm_calls): far rows like near rows, one cohort per stream
    int row_bytes;     // bytes of one stream's row in a slot: 172, or WMIX_PKG_SIZE
    int far_samples;   // int16 elements of the far-end of one step
    int pkt10, ppc;    // int16 elements of one 10 ms packet, packets per step
    wmx_chain *chain;
    wmx_rtp *snd;
    int16_t *d_pcm;        // [n][160] the 20 ms of every stream between ingest and egress
    uint32_t *d_nbytes;    // [n] what rtp_recv + G711a2PCM delivered (320 or 0)
    uint16_t *d_seq;       // [n] header sequence numbers as the reference leaves them
    // the slots (slot_ring.h): the rows in, the rows out (a PCM pipe works in place: out's device twin is in's) and the far-end of the
    // slot's step -- one package, or a row per stream -- for hosts that have it in host memory
    enum { kIn, kOut, kFar };
    wmx::SlotRing ring;
    long failed_steps;  // submits that failed after their first launch: the step is lost (slot_ring.h, FAILING CLEAN)
};

namespace wmx {
// rt.hip -> pipe.hip.  pipe_make with `s_in` / `s_out` given makes a sub-batch of a wmx_rt on the rt's copy streams.
int pipe_make(wmx_pipe **out, int n_streams, int slots, bool pcm, int law, int chn, int freq, int interval_ms, int agc_value, unsigned stages,
              hipStream_t s_in, hipStream_t s_out, bool far_rows = false);
// wmx_pipe_submit with two extras for a tick made of several sub-batches.  `flush_for` (NULL = h itself): the pipe whose pending
// download this submit queues behind ITS noise suppressor -- the previous sub-batch of the same tick; a download h itself still owes
// from an earlier tick is then queued first, ungated.  `far_of` (may be NULL): with d_far NULL, the pipe whose slot holds the tick's
// far-end on the device already (it went up once, with the first sub-batch): h uploads none and its chain reads that copy.
int pipe_submit(wmx_pipe *h, const int16_t *d_far, int *slot, void *stream, wmx_pipe *flush_for, const wmx_pipe *far_of);
}  // namespace wmx
