// tick.hip -- the daemon's 20 ms tick, play side and record side together, as ONE C call for many mixers (host code only: it
// sequences launches of mix.hip, pkgfifo.hip, chain.hip).
//
// With WMIX_RECORD_PLAY_SYNC (src/wmixConf.h:144, the shipped configuration) the play thread does, per package of
// WMIX_INTERVAL_MS (src/wmix.c:1347-1440):
//     drain WMIX_PKG_SIZE bytes at the ring head (copy out, zero, head and tick advance)          :1347-1366
//     playPkgBuff_add(playBuff)                                                                    :1419   (:480-491)
//     wmix_ao_write(playBuff)                                                                      :1421   -> d_play, the caller's
//     wmix_shmem_write_circle():                                                                   :1439   (:528-780)
//         buffSrc = wmix_ai_read()                                                                 :609    <- d_rec, the caller's
//         ns_process -> aec_process2(playPkgBuff_get(AEC_INTERVALMS), buffSrc, buffSrc, .., 0) -> agc_process -> vad_process
//                                                                                                  :613-709
//         wmix_pcm_zoom(WMIX_CHN, WMIX_FREQ, buffSrc, .., 1, 8000, buffDist)                       :730    -> d_rec_1x8000
// while the task threads put their sources into the ring with wmix_load_data (src/wmixTask.c:85, 973, 1311, 1484, 1704, 1927).
//
// A wmx_tick is G such daemons side by side: G rings (one mix group each), one FIFO slot row per group, and R record streams per
// group whose echo canceller hears THAT group's delayed playback -- one mix group = one far-end = one control cohort, so nothing
// folds (round-4 VERDICT "next" 3).  The record streams of group g are the rows g * R .. g * R + R - 1.
#include <vector>
#include "wmx_internal.h"
#include "bridge_layout.h"

struct wmx_tick {
    int device;  // first member of every handle (wmx_handle_device)
    int n_groups, rec_per_group, chn, freq, interval_ms, aec_delay_ms;
    int pkg;          // int16 elements of one package of one stream: freq / 1000 * interval_ms * chn  (WMIX_PKG_SIZE / 2)
    wmx_mix *mix;
    wmx_pkgfifo *fifo;
    wmx_chain *chain;
    wmx_ns *play_ns;  // WR_NS_PA: the playback's own noise suppressor (src/wmix.c:1370-1386), one stream per group; NULL = switched off
    int16_t *d_play;  // [n_groups][pkg] when the caller does not want the playback
    int16_t *d_far;   // [n_groups][pkg] playPkgBuff_get()'s packet of every group
    bool rw_test = false;                    // wmix->rwTest (src/wmix.c:714-732)
    uint32_t rw_head = UINT32_MAX, rw_tick = 0;  // rwTestHead / tick, the heartbeat's static cursor (:531-532)
    int bridge = 0;                              // wmx_tick_bridge: participants per conference, 0 = off
    uint32_t br_head = UINT32_MAX, br_tick = 0;  // the bridge's cursor: one for all pairs, they start together and move alike
    bool conf_on = false;                        // wmx_tick_bridge_conferences: a layout is in force
    std::vector<int32_t> conf_sizes;             // its conferences' sizes, for the carrying-over of the cursors
    std::vector<uint32_t> conf_head, conf_tick;  // one cursor per conference index
    uint8_t *d_mute = nullptr;                   // [n_groups] muted participants; nullptr = nobody
    std::vector<uint8_t> h_mute;                 // what the upload in flight reads
    int spk_max = 0, spk_shift = 0;              // wmx_tick_bridge_speakers: the loudest spk_max legs of a conference are loaded; 0 = off
    uint32_t spk_floor = 0;
    uint8_t *d_spk_mute = nullptr;               // [n_groups] the selection's mask, the bridge load's d_mute while it is on
};

extern "C" {

int wmx_tick_destroy(wmx_tick *h) {
    WMX_ON_DEVICE(h);
    if (!h) return 0;
    if (h->mix) wmx_mix_destroy(h->mix);
    if (h->fifo) wmx_pkgfifo_destroy(h->fifo);
    if (h->chain) wmx_chain_destroy(h->chain);
    if (h->play_ns) wmx_ns_destroy(h->play_ns);
    if (h->d_play) (void)hipFree(h->d_play);
    if (h->d_far) (void)hipFree(h->d_far);
    if (h->d_mute) (void)hipFree(h->d_mute);
    if (h->d_spk_mute) (void)hipFree(h->d_spk_mute);
    delete h;
    return 0;
}

int wmx_tick_create(wmx_tick **out, int n_groups, int rec_per_group, int chn, int freq, int interval_ms, int aec_delay_ms, int agc_value,
                    unsigned stages) {
    if (!out) return WMX_EINVAL;
    *out = nullptr;
    if (n_groups < 1 || rec_per_group < 1 || interval_ms < 10 || interval_ms % 10 || aec_delay_ms < 0 || aec_delay_ms % interval_ms) {
        // (a delay that is not a whole number of packages makes the reference's FIFO read a byte range that straddles two slots,
        // src/wmix.c:511-523; wmx_pkgfifo does that too, but no platform of the reference asks for it)
        wmx::set_error("wmx_tick_create: n_groups=%d rec_per_group=%d interval_ms=%d aec_delay_ms=%d", n_groups, rec_per_group, interval_ms,
                       aec_delay_ms);
        return WMX_EINVAL;
    }
    wmx_tick *h = new wmx_tick();
    if ((h->device = wmx::current_device()) < 0) {
        delete h;
        return WMX_ENODEV;
    }
    h->n_groups = n_groups;
    h->rec_per_group = rec_per_group;
    h->chn = chn;
    h->freq = freq;
    h->interval_ms = interval_ms;
    h->aec_delay_ms = aec_delay_ms;
    h->pkg = freq / 1000 * interval_ms * chn;
    int rc = wmx_mix_create(&h->mix, n_groups, chn, freq);
    // AEC_FIFO_PKG_NUM = AEC_INTERVALMS / WMIX_INTERVAL_MS + 2 slots of WMIX_PKG_SIZE bytes, src/wmixConf.h:141
    if (rc == 0) rc = wmx_pkgfifo_create(&h->fifo, n_groups, aec_delay_ms / interval_ms + 2, h->pkg * 2, interval_ms, chn * 2);
    if (rc == 0) {
        std::vector<int32_t> cohort((size_t)n_groups * rec_per_group);
        for (size_t s = 0; s < cohort.size(); s++) cohort[s] = (int32_t)(s / (size_t)rec_per_group);
        // one cohort per group only where a canceller needs it: without one the chain has no far-end at all
        const int nc = (stages & WMX_CHAIN_AEC) ? n_groups : 1;
        rc = wmx_chain_create_groups(&h->chain, n_groups * rec_per_group, chn, freq, interval_ms, agc_value, stages, nc,
                                     nc > 1 ? cohort.data() : nullptr);
        // a canceller that is switched on later (wmx_tick_set_stages) still hears one far-end per group
        if (rc == 0) wmx::chain_cohorts_when_made(h->chain, n_groups, n_groups > 1 ? cohort.data() : nullptr);
    }
    if (rc == 0) {
        hipError_t e = hipMalloc(&h->d_play, (size_t)n_groups * h->pkg * sizeof(int16_t));
        if (e == hipSuccess) e = hipMalloc(&h->d_far, (size_t)n_groups * h->pkg * sizeof(int16_t));
        if (e != hipSuccess) rc = wmx::hip_fail(e, "hipMalloc(tick buffers)", __FILE__, __LINE__);
    }
    if (rc != 0) {
        wmx_tick_destroy(h);
        return rc;
    }
    *out = h;
    return 0;
}

// The heartbeat's switches at run time: webrtcEnable[WR_VAD / WR_AEC / WR_NS / WR_AGC], which the daemon's message thread sets
// (src/wmix.c:1010-1050) -- and which the reference SHIPS as NS = 1, AGC = 1, VAD = 0, AEC = 0 (src/wmix.c:1580-1584).  A stage whose
// switch drops is released, one that comes on gets fresh handles in the next heartbeat (wmx_chain_set_stages); 0 = a pure
// mix / FIFO / zoom tick.  agc_value: agc_init's value for an AGC that comes on (the daemon: wmix->volumeAgc of that moment; < 0 keeps
// the tick's).  A control-plane call (the device is drained when a stage goes).
int wmx_tick_set_stages(wmx_tick *h, unsigned stages, int agc_value) { return h ? wmx_chain_set_stages(h->chain, stages, agc_value) : WMX_EINVAL; }

// The platform build's PLAT_PLAY_CORRECT (wmx_mix_set_play_correct); its PLAT_AEC_INTERVALMS is wmx_tick_create's aec_delay_ms.
int wmx_tick_set_play_correct(wmx_tick *h, uint32_t bytes) { return h ? wmx_mix_set_play_correct(h->mix, bytes) : WMX_EINVAL; }

// wmix->rwTest, the daemon's self send-receive test (src/wmix.c:714-732): while on, every heartbeat loads what it recorded -- the
// chain's output of the group's FIRST record stream, the daemon has one -- back into the group's play ring through wmix_load_data
// with a cursor of its own (reduce 1), so it is played VIEW_PLAY_CORRECT later, reaches the FIFO and comes back as far-end.  Off: the
// cursor is forgotten (rwTestHead = 0, tick = 0, :728-732).
int wmx_tick_rw_test(wmx_tick *h, int on) {
    if (!h) return WMX_EINVAL;
    if (on && (h->bridge || h->conf_on)) {
        wmx::set_error("wmx_tick_rw_test: the bridge is on (the two loads would feed the same rings)");
        return WMX_EINVAL;
    }
    h->rw_test = on != 0;
    if (!on) h->rw_head = UINT32_MAX, h->rw_tick = 0;
    return 0;
}

// The conference bridge: the tick's groups read as conferences of `parties` call legs.  A tick with rec_per_group == 1 already gives
// every group its own ring, FIFO row, far-end and control cohort; the bridge adds the one thing a room with one loudspeaker does not
// have: wmx_tick_record loads every participant's chain output into the rings of the others (wmx_mix_load_minus), where the rwTest
// load sits in the heartbeat (src/wmix.c:716-726).
int wmx_tick_bridge(wmx_tick *h, int parties) {
    if (!h) return WMX_EINVAL;
    if (parties == 0) {
        h->bridge = 0;
        h->br_head = UINT32_MAX, h->br_tick = 0;
        return 0;
    }
    if (parties < 2 || parties > WMX_MIX_MAX_PARTIES || h->n_groups % parties != 0 || h->rec_per_group != 1 || h->rw_test) {
        wmx::set_error("wmx_tick_bridge: parties=%d needs 2 .. %d, n_groups=%d a multiple of it, rec_per_group=%d == 1 and rwTest off", parties,
                       WMX_MIX_MAX_PARTIES, h->n_groups, h->rec_per_group);
        return WMX_EINVAL;
    }
    if (h->conf_on) {
        wmx::set_error("wmx_tick_bridge: a layout of wmx_tick_bridge_conferences is in force (the two loads would feed the same rings)");
        return WMX_EINVAL;
    }
    if (h->bridge != parties) h->br_head = UINT32_MAX, h->br_tick = 0;
    h->bridge = parties;
    return 0;
}

// The bridge over a layout (include/wmix_amd.h, bridge_layout.h): conferences of different sizes whose legs join and leave between
// ticks.  The mixer validates and keeps the layout; the tick keeps one cursor per conference index and carries it over.
int wmx_tick_bridge_conferences(wmx_tick *h, int n_conf, const int32_t *host_off, const int32_t *host_members, void *stream) {
    WMX_ON_DEVICE(h);
    if (!h) return WMX_EINVAL;
    if (n_conf == 0) {
        const int rc = wmx_mix_set_conferences(h->mix, 0, nullptr, nullptr, stream);
        if (rc) return rc;
        h->conf_on = false;
        h->conf_sizes.clear(), h->conf_head.clear(), h->conf_tick.clear();
        return 0;
    }
    if (h->rec_per_group != 1 || h->rw_test || h->bridge) {
        wmx::set_error("wmx_tick_bridge_conferences: needs rec_per_group=%d == 1, rwTest off and wmx_tick_bridge off", h->rec_per_group);
        return WMX_EINVAL;
    }
    wmx::BridgeLayout now;  // the sizes of the new layout; the mixer's own check is the one that refuses
    const int rc = wmx_mix_set_conferences(h->mix, n_conf, host_off, host_members, stream);
    if (rc) return rc;
    (void)wmx::bridge_layout_build(now, h->n_groups, n_conf, host_off, host_members);
    wmx::bridge_cursors_carry(h->conf_sizes, now, h->conf_head, h->conf_tick);
    h->conf_sizes.resize((size_t)n_conf);
    for (int c = 0; c < n_conf; c++) h->conf_sizes[(size_t)c] = now.size(c);
    h->conf_on = true;
    return 0;
}

int wmx_tick_bridge_mute(wmx_tick *h, const uint8_t *host_mask, void *stream) {
    WMX_ON_DEVICE(h);
    if (!h) return WMX_EINVAL;
    hipStream_t s = wmx::as_stream(stream);
    if (!h->d_mute) {
        if (!host_mask) return 0;
        WMX_HIP(hipMalloc(&h->d_mute, (size_t)h->n_groups));
    }
    // the copy's source is pageable memory of the handle: the previous upload must have left it before it is rewritten
    WMX_HIP(hipStreamSynchronize(s));
    if (host_mask)
        h->h_mute.assign(host_mask, host_mask + h->n_groups);
    else
        h->h_mute.assign((size_t)h->n_groups, 0);
    WMX_HIP(hipMemcpyAsync(h->d_mute, h->h_mute.data(), (size_t)h->n_groups, hipMemcpyHostToDevice, s));
    return 0;
}

// Talker selection (include/wmix_amd.h, speakers.h): while on and a bridge form is on, wmx_tick_record puts wmx_mix_select_speakers /
// _conf between the chain and the bridge load.  Off leaves the envelopes as they are.
int wmx_tick_bridge_speakers(wmx_tick *h, int max_speakers, uint32_t floor, int decay_shift) {
    WMX_ON_DEVICE(h);
    if (!h) return WMX_EINVAL;
    if (max_speakers < 0 || max_speakers > WMX_MIX_MAX_PARTIES || decay_shift < 0 || decay_shift > 31) {
        wmx::set_error("wmx_tick_bridge_speakers: max_speakers=%d must be 0 .. %d and decay_shift=%d 0 .. 31", max_speakers, WMX_MIX_MAX_PARTIES,
                       decay_shift);
        return WMX_EINVAL;
    }
    if (max_speakers && !h->d_spk_mute) WMX_HIP(hipMalloc(&h->d_spk_mute, (size_t)h->n_groups));
    h->spk_max = max_speakers;
    h->spk_floor = floor;
    h->spk_shift = decay_shift;
    return 0;
}

int wmx_tick_bridge_speaking(wmx_tick *h, uint8_t *host_speaking, uint32_t *host_env, void *stream) {
    return h ? wmx_mix_export_speakers(h->mix, host_env, host_speaking, stream) : WMX_EINVAL;
}

// webrtcEnable[WR_NS_PA] (src/wmix.c:1370-1386): the played package goes through ns_process on its way out -- BEFORE playPkgBuff_add,
// so the echo cancellers hear the suppressed playback too.  on = 1: ns_init of one suppressor per group (the switch coming on);
// on = 0: ns_release.
int wmx_tick_play_ns(wmx_tick *h, int on) {
    WMX_ON_DEVICE(h);
    if (!h) return WMX_EINVAL;
    if (!on) {
        if (h->play_ns) {
            WMX_HIP(hipDeviceSynchronize());
            wmx_ns_destroy(h->play_ns);
            h->play_ns = nullptr;
        }
        return 0;
    }
    if (h->play_ns) return 0;
    return wmx_ns_create(&h->play_ns, h->n_groups, h->chn, h->freq);
}

wmx_mix *wmx_tick_mix(wmx_tick *h) { return h ? h->mix : nullptr; }
wmx_chain *wmx_tick_chain(wmx_tick *h) { return h ? h->chain : nullptr; }
wmx_pkgfifo *wmx_tick_fifo(wmx_tick *h) { return h ? h->fifo : nullptr; }
int wmx_tick_package_samples(const wmx_tick *h) { return h ? h->pkg : WMX_EINVAL; }

// the task threads' wmix_load_data calls of this tick: wmx_mix_load on the tick's mixer (same arguments, same cursor rule)
int wmx_tick_load(wmx_tick *h, const int16_t *d_src, uint32_t srcU8Len, int freq, int channels, int sample, int n_src, long group_stride,
                  long source_stride, int reduce, uint32_t *head, uint32_t *tick, void *stream) {
    if (!h) return WMX_EINVAL;
    return wmx_mix_load(h->mix, d_src, srcU8Len, freq, channels, sample, n_src, group_stride, source_stride, reduce, head, tick, stream);
}

// The play side of one package (src/wmix.c:1347-1421): drain -> playPkgBuff_add -> what goes to the sound card (d_play, may be NULL:
// n_groups rows, play_stride int16 apart) -- and playPkgBuff_get(AEC_INTERVALMS) into the tick's far-end rows, which the record side
// of the same package will hand the echo cancellers (the daemon fetches it inside the heartbeat, :651; the FIFO does not move in
// between, so fetching it here is the same packet).
int wmx_tick_play(wmx_tick *h, int16_t *d_play, long play_stride, void *stream) {
    WMX_ON_DEVICE(h);
    if (!h || (d_play && play_stride < h->pkg)) {
        wmx::set_error("wmx_tick_play: bad argument");
        return WMX_EINVAL;
    }
    int16_t *play = d_play ? d_play : h->d_play;
    const long pstride = d_play ? play_stride : (long)h->pkg;
    const uint32_t pkg_bytes = (uint32_t)h->pkg * 2;
    int rc = wmx_mix_drain(h->mix, play, pkg_bytes, pstride, stream);
    if (rc == 0 && h->play_ns) {
        const int pkg10 = h->freq / 100 * h->chn;
        rc = wmx_ns_process(h->play_ns, play, play, h->interval_ms / 10, pstride, pkg10, stream);
    }
    if (rc == 0) rc = wmx_pkgfifo_add(h->fifo, reinterpret_cast<const uint8_t *>(play), pstride * 2, stream);
    if (rc == 0) rc = wmx_pkgfifo_get(h->fifo, reinterpret_cast<uint8_t *>(h->d_far), (long)pkg_bytes, h->aec_delay_ms, stream);
    return rc;
}

// the far-end package of every group as wmx_tick_play left it: [n_groups][package] int16 on the device (a harness that models the
// room -- loudspeaker into microphone -- reads it between the two halves of a tick)
const int16_t *wmx_tick_far(const wmx_tick *h) { return h ? h->d_far : nullptr; }

// The record side of the package = wmix_shmem_write_circle (src/wmix.c:528-780) for every record stream.  d_rec: n_groups *
// rec_per_group rows of one package each, rec_stride apart: the captured audio in, the chain's output out (in place, like buffSrc).
// d_rec_1x8000 (may be NULL): rows of out_capacity bytes, out_stride int16 apart, receive wmix_pcm_zoom(.., 1, 8000); *out_len the
// bytes written per row.
int wmx_tick_record(wmx_tick *h, int16_t *d_rec, long rec_stride, int16_t *d_rec_1x8000, long out_stride, uint32_t out_capacity,
                    uint32_t *out_len, void *stream) {
    WMX_ON_DEVICE(h);
    if (!h || !d_rec || rec_stride < h->pkg) {
        wmx::set_error("wmx_tick_record: bad argument");
        return WMX_EINVAL;
    }
    const int pkg10 = h->freq / 100 * h->chn;
    int rc = wmx_chain_process_groups(h->chain, h->d_far, pkg10, h->pkg, d_rec, d_rec, h->interval_ms / 10, rec_stride, pkg10, nullptr, nullptr,
                                      nullptr, stream);
    if (rc != 0) return rc;
    if (h->rw_test) {  // :716-726: buffSrc, `ret` bytes, WMIX_FREQ x WMIX_CHN x WMIX_SAMPLE, rwTestHead, reduce 1, &tick
        rc = wmx_mix_load(h->mix, d_rec, (uint32_t)h->pkg * 2, h->freq, h->chn, 16, 1, (long)h->rec_per_group * rec_stride, 0, 1, &h->rw_head,
                          &h->rw_tick, stream);
        if (rc != 0) return rc;
    }
    const uint8_t *load_mute = h->d_mute;
    if (h->spk_max && (h->bridge || h->conf_on)) {  // who is loaded this tick: decided on the chain's output, where it lies
        if (h->bridge)
            rc = wmx_mix_select_speakers(h->mix, h->bridge, d_rec, (uint32_t)h->pkg * 2, (long)h->bridge * rec_stride, rec_stride, h->d_mute,
                                         h->spk_max, h->spk_floor, h->spk_shift, h->d_spk_mute, stream);
        else
            rc = wmx_mix_select_speakers_conf(h->mix, d_rec, (uint32_t)h->pkg * 2, rec_stride, h->d_mute, h->spk_max, h->spk_floor, h->spk_shift,
                                              h->d_spk_mute, stream);
        if (rc != 0) return rc;
        load_mute = h->d_spk_mute;
    }
    if (h->bridge) {  // every leg's output into the rings of the other legs of its conference
        rc = wmx_mix_load_minus(h->mix, h->bridge, d_rec, (uint32_t)h->pkg * 2, h->freq, h->chn, 16, (long)h->bridge * rec_stride, rec_stride,
                                load_mute, 1, &h->br_head, &h->br_tick, stream);
        if (rc != 0) return rc;
    }
    if (h->conf_on) {  // the same over the layout, every conference from its own cursor
        rc = wmx_mix_load_minus_conf(h->mix, d_rec, (uint32_t)h->pkg * 2, h->freq, h->chn, 16, rec_stride, load_mute, 1, h->conf_head.data(),
                                     h->conf_tick.data(), stream);
        if (rc != 0) return rc;
    }
    if (d_rec_1x8000) {
        uint32_t got = 0;
        rc = wmx_pcm_zoom(h->chn, h->freq, d_rec, (uint32_t)h->pkg * 2, 1, 8000, d_rec_1x8000, out_capacity, rec_stride, out_stride,
                          h->n_groups * h->rec_per_group, &got, stream);
        if (out_len) *out_len = got;
    }
    return rc;
}

// One whole package: the play side, then the record side on audio that was captured beforehand.
int wmx_tick_run(wmx_tick *h, int16_t *d_play, long play_stride, int16_t *d_rec, long rec_stride, int16_t *d_rec_1x8000, long out_stride,
                 uint32_t out_capacity, uint32_t *out_len, void *stream) {
    const int rc = wmx_tick_play(h, d_play, play_stride, stream);
    return rc ? rc : wmx_tick_record(h, d_rec, rec_stride, d_rec_1x8000, out_stride, out_capacity, out_len, stream);
}

}  // extern "C"
