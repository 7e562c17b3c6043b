// cohort_hip.h -- the device half of the cohort machinery of aec.hip and aecm.hip (the host bookkeeping is cohort_reg.h).
//
// CohortDev adds to the registry what lives on the device or in HIP objects: the far-end slabs, plan_of, the plan slots, the
// coalescing flags and the far-kernel fork.  run_cohorts / coalesce: the entry points' bodies, given the module's kernel launches.
#pragma once
#include <type_traits>
#include "cohort_reg.h"
#include "stage_life.h"  // the blob header (and wmx_internal.h)

namespace wmx {

// one launch of a run: its plans ([packet][class], C apart, in the pinned slot hp and the device slot dp) and its first packet
template <class Plan>
struct CohortLaunch {
    Plan *hp, *dp;
    int chunk, C, G, done, by_value;
    const int32_t *plan_of;  // nullptr with one cohort
};

template <class Ctl, class Pairs, int kSlots>
struct CohortDev : CohortReg<Ctl, Pairs> {
    using Plan = typename Ctl::Plan;
    using PairList = Pairs;
    static constexpr int kPlanSlots = kSlots, kMaxPkt = Ctl::kMaxPktPerLaunch;
    int cap = 0;                   // cohorts the device buffers (far slabs, plan slots, plan_of) are allocated for; grows by doubling
    size_t slab_bytes = 0;         // one cohort's far-end slab
    void *d_far = nullptr;         // [cap] slabs
    int32_t *d_plan_of = nullptr;  // [cap] class index of every cohort
    // plan slots: kSlots x [kMaxPktPerLaunch][cap] plans, used round robin (a launch uses the first chunk x C plans of its slot); the
    // pinned mirror is read by the asynchronous copy in place, so each slot has its own
    Plan *d_plans = nullptr, *h_plans = nullptr;
    hipEvent_t plan_free[kSlots] = {};  // recorded behind the kernels that read slot i; waited for before slot i is rewritten
    bool plan_used[kSlots] = {};
    int plan_sel = 0;
    int *d_co_flags = nullptr, *h_co_flags = nullptr;  // [kCoMax] the comparison's result and its pinned copy
    hipEvent_t co_done = nullptr;
    bool co_inflight = false;
    // The far kernel is one wave per cohort and needs nothing but the far-end packet: a caller that has other work for the GPU in
    // front of the near kernel (wmx_chain_process: the noise suppressor) lets it run BESIDE that work on this side stream instead
    // of alone in front of the near kernel (fork_far).
    hipStream_t side = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    bool fork_pending = false;

    char *slab(int g) const { return static_cast<char *>(d_far) + (size_t)g * slab_bytes; }

    void release() {
        if (d_far) (void)hipFree(d_far);
        if (d_plan_of) (void)hipFree(d_plan_of);
        if (d_plans) (void)hipFree(d_plans);
        if (h_plans) (void)hipHostFree(h_plans);
        if (d_co_flags) (void)hipFree(d_co_flags);
        if (h_co_flags) (void)hipHostFree(h_co_flags);
        if (co_done) (void)hipEventDestroy(co_done);
        if (side) (void)hipStreamDestroy(side);
        if (ev_fork) (void)hipEventDestroy(ev_fork);
        if (ev_join) (void)hipEventDestroy(ev_join);
        for (int i = 0; i < kSlots; i++)
            if (plan_free[i]) (void)hipEventDestroy(plan_free[i]);
    }

    // Device buffers for `want` cohorts: the far-end slabs (existing ones carried over, new ones zeroed), plan_of and the plan slots;
    // carve() then lays the module's buffers over d_far.  Growing is a control-plane operation (the device is drained); it doubles,
    // so a batch that gains cohorts one join at a time reallocates a logarithmic number of times.
    template <class Carve>
    int reserve(int want, Carve carve) {
        if (want <= cap) return 0;
        WMX_HIP(hipDeviceSynchronize());  // plans and far slabs may be in use by launches in flight
        int ncap = cap > 0 ? cap : 1;
        while (ncap < want) ncap *= 2;
        // everything new is allocated BEFORE anything old is let go: a failure leaves the handle as it was
        void *nf = nullptr;
        Plan *nd = nullptr, *nh = nullptr;
        int32_t *npo = nullptr;
        const size_t plan_bytes = (size_t)kSlots * ncap * kMaxPkt * sizeof(Plan);
        hipError_t e = hipMalloc(&nf, slab_bytes * (size_t)ncap);
        if (e == hipSuccess) e = hipMalloc(&nd, plan_bytes);
        if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void **>(&nh), plan_bytes, hipHostMallocDefault);
        if (e == hipSuccess) e = hipMalloc(&npo, sizeof(int32_t) * (size_t)ncap);
        if (e == hipSuccess && d_far) e = hipMemcpy(nf, d_far, slab_bytes * (size_t)cap, hipMemcpyDeviceToDevice);
        if (e == hipSuccess) e = hipMemset(static_cast<char *>(nf) + slab_bytes * (size_t)cap, 0, slab_bytes * (size_t)(ncap - cap));
        if (e != hipSuccess) {
            if (nf) (void)hipFree(nf);
            if (nd) (void)hipFree(nd);
            if (nh) (void)hipHostFree(nh);
            if (npo) (void)hipFree(npo);
            return hip_fail(e, "growing the cohort buffers", __FILE__, __LINE__);
        }
        if (d_far) (void)hipFree(d_far);
        if (d_plans) (void)hipFree(d_plans);
        if (h_plans) (void)hipHostFree(h_plans);
        if (d_plan_of) (void)hipFree(d_plan_of);
        d_plan_of = npo;
        this->cls_dirty = true;  // the new array holds nothing yet
        d_far = nf;
        d_plans = nd;
        h_plans = nh;
        for (int i = 0; i < kSlots; i++) plan_used[i] = false;  // drained above
        cap = ncap;
        carve();
        return 0;
    }
    // A new cohort (wmx_*_add_cohort): a retired id when there is one, else the next, the buffers grown for it; *d_map (the device's
    // stream -> cohort map) is made when a second cohort appears -- so far every stream was in cohort 0 by construction.  The caller
    // restarts the cohort.
    template <class Carve>
    int add(int *&d_map, int n_streams, hipStream_t s, int *id_out, Carve carve) {
        if (this->free_id() == this->n()) {
            const int rc = reserve(this->n() + 1, carve);
            if (rc != 0) return rc;
        }
        *id_out = this->take_id();
        if (this->n() > 1 && !d_map) {
            WMX_HIP(hipMalloc(&d_map, sizeof(int) * n_streams));
            WMX_HIP(hipMemsetAsync(d_map, 0, sizeof(int) * n_streams, s));
        }
        return 0;
    }
    // wmx_*_reset_cohort: the control plane starts over and the cohort's far-end slab is cleared
    int reset(int g, hipStream_t s) {
        this->restart(g);
        WMX_HIP(hipMemsetAsync(slab(g), 0, slab_bytes, s));
        return 0;
    }
    // The cohort blob: [header | Ctl | slab]; a destination cohort that received it continues exactly where the source cohort stands.
    int blob_bytes() const { return (int)(sizeof(BlobHeader) + sizeof(Ctl) + slab_bytes); }
    int export_blob(int g, uint32_t tag, uint32_t layout, void *blob) {
        WMX_HIP(hipDeviceSynchronize());
        char *p = static_cast<char *>(blob);
        blob_begin(p, tag, layout, (uint32_t)(sizeof(Ctl) + slab_bytes));
        p += sizeof(BlobHeader);
        memcpy(p, &this->plane(g), sizeof(Ctl));
        WMX_HIP(hipMemcpy(p + sizeof(Ctl), slab(g), slab_bytes, hipMemcpyDeviceToHost));
        return 0;
    }
    int import_blob(int g, uint32_t tag, uint32_t layout, const void *blob) {
        const int rc = blob_check(blob, tag, layout, (uint32_t)(sizeof(Ctl) + slab_bytes));
        if (rc) return rc;
        WMX_HIP(hipDeviceSynchronize());
        const char *p = static_cast<const char *>(blob) + sizeof(BlobHeader);
        Ctl c;
        memcpy(&c, p, sizeof(Ctl));
        this->import(g, c);
        WMX_HIP(hipMemcpy(slab(g), p + sizeof(Ctl), slab_bytes, hipMemcpyHostToDevice));
        return 0;
    }
    // from this point of `s` on, the far-end packets of the next run are in place: its far kernel may start here, on the side stream
    int fork(hipStream_t s) {
        if (!side) {
            WMX_HIP(hipStreamCreateWithFlags(&side, hipStreamNonBlocking));
            WMX_HIP(hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming));
            WMX_HIP(hipEventCreateWithFlags(&ev_join, hipEventDisableTiming));
        }
        WMX_HIP(hipEventRecord(ev_fork, s));
        fork_pending = true;
        return 0;
    }
    // cls_leader / plan_of from lead[], and plan_of onto the device in `s` (alternating host sources, like the AEC's stream order)
    int upload_classes(hipStream_t s) {
        const std::vector<int32_t> &po = this->list_classes();
        if (this->n() > 1) WMX_HIP(hipMemcpyAsync(d_plan_of, po.data(), sizeof(int32_t) * (size_t)this->n(), hipMemcpyHostToDevice, s));
        this->cls_dirty = false;
        return 0;
    }
};

// Library-internal (wmx_internal.h): wmx::aec_fork_far / aecm_fork_far
template <class H>
int fork_far(H *h, hipStream_t s) {
    WMX_ON_DEVICE(h);
    if (!h) return WMX_EINVAL;
    return h->co.fork(s);
}
// wmx_*_reset_cohort, _retire_cohort and _cohort_key: their argument checks around the shared code
template <class H>
int reset_cohort(H *h, int cohort, void *stream) {
    WMX_ON_DEVICE(h);
    if (!h || cohort < 0 || cohort >= h->co.n()) return WMX_EINVAL;
    return h->co.reset(cohort, as_stream(stream));  // cohorts restarted at the same point of the packet sequence run one control plane
}
template <class H>
int retire_cohort(H *h, int cohort) {
    if (!h || cohort < 0 || cohort >= h->co.n()) return WMX_EINVAL;
    h->co.retire(cohort);
    return 0;
}
template <class H>
int cohort_key(const H *h, int cohort, int32_t *key) {
    if (!h || !key || cohort < 0 || cohort >= h->co.n()) return WMX_EINVAL;
    return h->co.key(cohort, key);  // 1: retired, or still in its start-up
}

// The body of wmx_*_run_cohorts behind the module's null check (H: the handle, its cohorts in h->co).  The module's part, no virtual
// calls: before(running) does everything else that can fail before a plane moves; plan(loop) runs loop(), the planning of one launch,
// and returns its result; far(fs, L) uploads the plans (where they are not read otherwise) and launches the far kernel in fs;
// near(L) launches the near kernel (mode & 2).
template <class H, class Before, class PlanLoop, class Far, class Near>
int run_cohorts(H *h, const char *name, int mode, const int16_t *d_far, long far_packet_stride, long far_group_stride, const int16_t *d_near,
                const int16_t *d_out, int n_packets, long stream_stride, long packet_stride, const int32_t *delay_ms, const uint8_t *cohort_on,
                int32_t *cohort_rc, hipStream_t s, Before before, PlanLoop plan, Far far, Near near) {
    auto &co = h->co;
    using Dev = typename std::remove_reference<decltype(co)>::type;
    // a fork point (fork_far) belongs to THIS call, whichever way it ends: taken over here, used by the first chunk that launches, and
    // gone on every other path (argument errors, every cohort switched off) -- a later call must not start its far kernel on the side
    // stream behind a stale event (round-3 ADVICE)
    const bool fork_here = co.fork_pending;
    co.fork_pending = false;
    if (n_packets < 0 || (mode & 3) == 0 || !delay_ms) {
        set_error("%s: bad argument", name);
        return WMX_EINVAL;
    }
    const int G = co.n();
    if (cohort_rc)
        for (int g = 0; g < G; g++) cohort_rc[g] = 0;
    if (n_packets == 0) return 0;  // frameNum == 0: nothing to do, whatever the pointers are
    if (((mode & 1) && !d_far) || ((mode & 2) && (!d_near || !d_out))) {
        set_error("%s: null buffer", name);
        return WMX_EINVAL;
    }
    const long per_pkt = (long)h->pkg * h->chn;
    if ((mode & 2) && (packet_stride < per_pkt || (h->n_streams > 1 && stream_stride < per_pkt))) {
        set_error("%s: strides (%ld, %ld) smaller than a packet (%ld samples)", name, stream_stride, packet_stride, per_pkt);
        return WMX_EINVAL;
    }
    if ((mode & 1) && far_packet_stride < per_pkt && n_packets > 1) {
        set_error("%s: far stride %ld smaller than a packet (%ld samples)", name, far_packet_stride, per_pkt);
        return WMX_EINVAL;
    }
    int rc_first = 0, running = co.begin_run(mode, far_group_stride, delay_ms, cohort_on);
    // Everything that can fail for lack of memory happens HERE, before a control plane has moved: a call that returns an error has
    // advanced neither the host's planes nor the device's far-end history (round-4 ADVICE: the AEC's stream order used to be
    // rebuilt -- an allocation and an upload -- between the far and the near kernel of a chunk whose planes had already been advanced).
    int rc;
    if ((rc = before(running)) != 0) return rc;
    // Control-plane classes: a follower that is called differently from its leader in THIS call (switched on / off alone, another
    // reported delay) takes a plane of its own first.  (wmx_*_run / _run_groups hand every cohort the same delay and no switches.)
    if (G > 1 && (cohort_on || delay_ms != co.same_delay.data())) co.split(delay_ms, cohort_on);
    bool classes_moved = false;
    if (co.cls_dirty) {
        // uploaded in `s`, behind every launch that still reads the old classes; a far kernel forked onto the side stream would not
        // wait for it (its fork point lies in front of this call): this one launch keeps the far kernel in line
        if ((rc = co.upload_classes(s)) != 0) return rc;
        classes_moved = true;
    }
    const int C = (int)co.cls_leader.size();
    const int32_t *plan_of = G > 1 ? co.d_plan_of : nullptr;
    running = co.running_classes(cohort_on);
    for (int done = 0; done < n_packets && running > 0;) {
        int chunk = n_packets - done;
        if (chunk > Dev::kMaxPkt) chunk = Dev::kMaxPkt;
        // the next plan slot: its pinned host half and its device half are rewritten only after the kernels that read the device
        // half last have finished, whatever stream they ran on (round-1 ADVICE: the single buffer was reused blindly)
        const int sel = co.plan_sel;
        co.plan_sel = (sel + 1) % Dev::kPlanSlots;
        if (co.plan_used[sel]) WMX_HIP(hipEventSynchronize(co.plan_free[sel]));
        const size_t slot = (size_t)sel * co.cap * Dev::kMaxPkt;
        const int by_value = (chunk == 1 && C == 1 && G == 1) ? 1 : 0;  // one plan: the far kernel takes it as an argument
        const CohortLaunch<typename Dev::Plan> L{co.h_plans + slot, co.d_plans + slot, chunk, C, G, done, by_value, plan_of};
        const int any = plan([&] { return co.plan_chunk(L.hp, chunk, mode, h->pkg, delay_ms, cohort_on, &running, &rc_first); });
        if (any) {
            // the far kernel (and the plans it reads) on the side stream when the caller forked it (first chunk of the call only)
            const bool forked = fork_here && done == 0 && (mode & 2) && !classes_moved;
            hipStream_t fs = forked ? co.side : s;
            if (forked) WMX_HIP(hipStreamWaitEvent(fs, co.ev_fork, 0));
            if ((rc = far(fs, L)) != 0) return rc;
            if (forked) {
                WMX_HIP(hipEventRecord(co.ev_join, fs));
                WMX_HIP(hipStreamWaitEvent(s, co.ev_join, 0));
            }
            if ((mode & 2) && (rc = near(L)) != 0) return rc;
            WMX_HIP(hipEventRecord(co.plan_free[sel], s));
            co.plan_used[sel] = true;
        }
        done += chunk;
    }
    co.end_run(cohort_on, cohort_rc);
    return rc_first;
}

// The body of wmx_*_coalesce behind WMX_ON_DEVICE (include/wmix_amd.h).  Each call first completes the merges whose device
// comparison -- requested by an earlier call -- came back equal, then proposes up to max_pairs new pairs and launches their
// comparison behind the work already in `stream`.  Nothing here waits for the device.  The module launches its kernels:
//     int merge(const Pairs &go, int n_go, hipStream_t s)   the merge itself, then co.retire_merged / co.shrink (its clamp kernel)
//     void equal(int n, hipStream_t s)                      launches the comparison of co.co_pairs.p[0, n) into co.d_co_flags
template <class H, class Merge, class Equal>
int coalesce(H *h, int max_pairs, int32_t *merged_from, int32_t *merged_into, int cap, int *n_merged, void *stream, const int *d_map,
             Merge merge, Equal equal) {
    if (n_merged) *n_merged = 0;
    if (!h || max_pairs < 0 || cap < 0 || (cap > 0 && (!merged_from || !merged_into))) return WMX_EINVAL;
    auto &co = h->co;
    using Dev = typename std::remove_reference<decltype(co)>::type;
    hipStream_t s = as_stream(stream);
    co.co_calls++;
    if (co.n() < 2 || !d_map) return 0;
    if (!co.d_co_flags) {
        WMX_HIP(hipMalloc(&co.d_co_flags, sizeof(int) * Dev::kCoMax));
        WMX_HIP(hipHostMalloc(reinterpret_cast<void **>(&co.h_co_flags), sizeof(int) * Dev::kCoMax, hipHostMallocDefault));
        WMX_HIP(hipEventCreateWithFlags(&co.co_done, hipEventDisableTiming));
    }
    int merged = 0;
    if (co.co_inflight) {
        const hipError_t q = hipEventQuery(co.co_done);
        if (q == hipErrorNotReady) return 0;  // the comparison has not run yet: nothing new is proposed on top of it
        if (q != hipSuccess) return hip_fail(q, "hipEventQuery(co_done)", __FILE__, __LINE__);
        co.co_inflight = false;
        typename Dev::PairList go;
        merged = co.collect(co.h_co_flags, merged_from, merged_into, cap, go.p);
        int rc;
        if (merged > 0 && (rc = merge(go, merged, s)) != 0) return rc;
    }
    if (n_merged) *n_merged = merged;
    const int n = co.propose(max_pairs);
    if (n == 0) return 0;
    equal(n, s);
    WMX_LAUNCH_CHECK();
    WMX_HIP(hipMemcpyAsync(co.h_co_flags, co.d_co_flags, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, s));
    WMX_HIP(hipEventRecord(co.co_done, s));
    co.co_inflight = true;
    return 0;
}

}  // namespace wmx
