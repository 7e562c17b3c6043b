// cohort_reg.h -- the control cohorts of a batched echo canceller: host bookkeeping, no HIP.
//
// A cohort is a group of streams that share one control plane and one far-end history (aec.hip, aecm.hip).  CohortReg<Ctl, Pairs>
// keeps the per-cohort host arrays of either canceller (Ctl: AecCtl or AecmCtl) and everything done with them: ids handed out,
// retired, restarted and imported over, the control-plane classes, the planning loop of a launch and the host half of coalescing.
// Where the two cancellers differ, Ctl's header has an overload: co_key / co_pair, plan_clear / plan_reject_near; Ctl::Plan, Key and
// Pair name its types.  Pairs is the module's pair list (the argument of its comparison and merge kernels): its length is the number
// of pairs per comparison and merges per call.  The device half is cohort_hip.h.
#pragma once
#include <algorithm>
#include <cstdint>
#include <unordered_map>
#include <vector>

namespace wmx {

template <class Ctl, class Pairs>
struct CohortReg {
    using Plan = typename Ctl::Plan;
    using Key = typename Ctl::Key;
    using Pair = typename Ctl::Pair;
    static constexpr int kCoMax = (int)(sizeof(Pairs::p) / sizeof(Pairs::p[0]));

    int freq = 0;
    std::vector<Ctl> ctl;  // one control plane per cohort id -- of which only the LEADERS' are kept up to date, see `lead`
    // Control-plane classes.  A control plane is index arithmetic on the call pattern (when the handle was made, packet sizes,
    // reported delays), never on audio: cohorts that were started at the same point and are called alike have EQUAL planes for ever
    // -- every mix group of a conference server started together, every call set up in the same tick -- although their far-ends
    // (and so their far-end histories on the device) differ and they can never be merged.  Such cohorts form a class: lead[g] is
    // the cohort whose plane stands for g's (lead[g] == g: g leads); a launch runs ONE control plane and uploads ONE plan per class
    // and packet, and the kernels find a cohort's plan through plan_of.  ctl[g] of a follower is stale; plane() reads through,
    // own() makes a cohort the owner of an up-to-date copy before anything treats it differently from its class.
    std::vector<int32_t> lead;          // [n()]
    std::vector<int32_t> cls_leader;    // [n_cls] the leaders, compact
    std::vector<int32_t> h_plan_of[2];  // [n()] class index of every cohort; alternating sources of the asynchronous upload
    int h_plan_of_sel = 0;
    bool cls_dirty = true;              // lead[] changed: cls_leader / plan_of are rebuilt (and uploaded) by the next launch
    std::vector<uint8_t> live;          // [n()] 0: retired (never called, its id is handed out again)
    // coalescing: the pairs whose device comparison is in flight (`b` < 0: dropped, the two were not called identically since)
    Pairs co_pairs;
    int co_n = 0;
    long co_calls = 0;               // coalesce calls so far
    std::vector<long> co_retry_at;   // [n()] a cohort whose comparison failed is not proposed again before this call
    long last_far_group_stride = 0;  // of the latest run: cohorts that hear private far-end packets are never candidates
    std::vector<int32_t> co_into;    // [n()] of the latest merge: the cohort each merged one went into, -1 for the others
    // per-call scratch kept with the handle (no allocation on the heartbeat's path)
    std::vector<int> rc_g;            // [n()] what the wrapper would have returned to the members of each cohort
    std::vector<int32_t> same_delay;  // [n()] the one reported delay of wmx_*_run / _run_groups, spread over the cohorts

    int n() const { return (int)lead.size(); }  // cohort ids in use, retired ones included
    // wmx_*_run / _run_groups: every cohort reports the same delay
    const int32_t *same_delays(int delay_ms) {
        same_delay.assign((size_t)n(), delay_ms);
        return same_delay.data();
    }
    const Ctl &plane(int g) const { return ctl[(size_t)lead[(size_t)g]]; }
    bool on(const uint8_t *cohort_on, int g) const { return live[(size_t)g] && (!cohort_on || cohort_on[g]); }

    // n cohorts made together: equal planes, one class led by cohort 0 until something tells them apart
    void init(int n_cohorts, int f) {
        freq = f;
        ctl.resize((size_t)n_cohorts);
        for (Ctl &c : ctl) c.init(freq);
        lead.assign((size_t)n_cohorts, 0);
        cls_dirty = true;
        live.assign((size_t)n_cohorts, 1);
        co_retry_at.assign((size_t)n_cohorts, 0);
    }

    // ---- ids
    // the id a new cohort gets: a retired one when there is one, else n() -- a new id at the end, for which the caller makes room
    int free_id() const {
        for (int g = 0; g < n(); g++)
            if (!live[(size_t)g]) return g;
        return n();
    }
    // that id, live from now on (the caller restarts its plane)
    int take_id() {
        const int id = free_id();
        if (id == n()) {
            ctl.resize((size_t)id + 1);
            lead.push_back(id);
            cls_dirty = true;
            live.push_back(1);
            co_retry_at.push_back(0);
        }
        live[(size_t)id] = 1;
        return id;
    }
    // never called again; its id may be handed out later
    void retire(int g) {
        own(g);  // a retired cohort leads nobody
        live[(size_t)g] = 0;
        drop(g);
    }
    // aec_init of the cohort's shared part: its plane starts over, and runs with the cohorts restarted at the same point
    void restart(int g) {
        Ctl c;
        c.init(freq);
        import(g, c);
    }
    // a plane of its own, that of a cohort blob or a fresh one
    void import(int g, const Ctl c) {
        own(g);
        ctl[(size_t)g] = c;
        join(g);
        drop(g);
    }
    int live_count() const { return (int)std::count(live.begin(), live.end(), 1); }
    // the coalescing key of a live cohort into out: 0, or 1 when it is retired or still in its start-up
    int key(int g, int32_t *out) const {
        Key k;
        if (!live[(size_t)g] || !co_key(plane(g), &k)) return 1;
        for (int i = 0; i < (int)(sizeof(k.v) / sizeof(k.v[0])); i++) out[i] = k.v[i];
        return 0;
    }

    // ---- classes
    // cohort g leaves its class with an up-to-date plane of its own (a leader hands the class over to its first follower)
    void own(int g) {
        const int l = lead[(size_t)g];
        if (l != g) {
            ctl[(size_t)g] = ctl[(size_t)l];
            lead[(size_t)g] = g;
            cls_dirty = true;
            return;
        }
        int heir = -1;
        for (int x = 0; x < n(); x++)
            if (x != g && lead[(size_t)x] == g) {
                if (heir < 0) {
                    heir = x;
                    ctl[(size_t)x] = ctl[(size_t)g];
                }
                lead[(size_t)x] = heir;
                cls_dirty = true;
            }
    }
    // cohort g (a leader of itself alone, its plane just rewritten: restart, import) joins a class whose plane is equal, if one of
    // the first few hundred leaders has it -- planes made at the same point of the packet sequence (a bounded search: a miss costs
    // a control plane of its own, nothing else)
    void join(int g) {
        int seen = 0;
        for (int x = 0; x < n() && seen < 256; x++) {
            if (x == g || lead[(size_t)x] != x || !live[(size_t)x]) continue;
            seen++;
            if (ctl[(size_t)x].same_as(ctl[(size_t)g])) {
                lead[(size_t)g] = x;
                cls_dirty = true;
                return;
            }
        }
    }
    // in front of a launch: a follower that is called differently from its leader in THIS call (switched on / off alone, another
    // reported delay) takes a plane of its own first.  cohort_on may be null (all on).
    void split(const int32_t *delay_ms, const uint8_t *cohort_on) {
        for (int g = 0; g < n(); g++) {
            const int l = lead[(size_t)g];
            if (l == g || !live[(size_t)g]) continue;
            const bool on_g = !cohort_on || cohort_on[g], on_l = !cohort_on || cohort_on[l];
            if (on_g != on_l || (on_g && delay_ms[g] != delay_ms[l])) own(g);
        }
    }
    // the leaders, compact, into cls_leader, and every cohort's class index into the next plan_of source, which is returned;
    // cls_dirty is cleared by the caller once the upload is queued
    const std::vector<int32_t> &list_classes() {
        h_plan_of_sel ^= 1;
        std::vector<int32_t> &plan_of = h_plan_of[h_plan_of_sel];
        const int G = n();
        plan_of.assign((size_t)G, 0);
        cls_leader.clear();
        for (int g = 0; g < G; g++)
            if (lead[(size_t)g] == g) {
                plan_of[(size_t)g] = (int32_t)cls_leader.size();
                cls_leader.push_back(g);
            }
        for (int g = 0; g < G; g++) plan_of[(size_t)g] = plan_of[(size_t)lead[(size_t)g]];
        return plan_of;
    }

    // ---- a run (wmx_*_run_cohorts)
    // rc_g cleared, the far-end group stride noted, and pairs whose comparison is in flight stay candidates only while the two
    // cohorts are called identically.  Returns the cohorts called.
    int begin_run(int mode, long far_group_stride, const int32_t *delay_ms, const uint8_t *cohort_on) {
        rc_g.assign((size_t)n(), 0);
        int running = 0;
        for (int g = 0; g < n(); g++) running += on(cohort_on, g) ? 1 : 0;
        last_far_group_stride = (mode & 1) ? far_group_stride : last_far_group_stride;
        for (int i = 0; i < co_n; i++) {
            Pair &pc = co_pairs.p[i];
            if (pc.b < 0) continue;
            const bool on_a = !cohort_on || cohort_on[pc.a], on_b = !cohort_on || cohort_on[pc.b];
            if (on_a != on_b || (on_a && delay_ms[pc.a] != delay_ms[pc.b]) || ((mode & 1) && far_group_stride != 0)) pc.b = -1;
        }
        return running;
    }
    int running_classes(const uint8_t *cohort_on) const {
        int running = 0;
        for (int32_t g : cls_leader) running += on(cohort_on, g) ? 1 : 0;
        return running;
    }
    // One launch's plans, [packet][class]: each class's one plane runs `chunk` packets.  A class whose call was rejected runs
    // nothing after the offending packet: *running loses it, *rc_first takes the first code.  Returns whether any packet runs.
    int plan_chunk(Plan *hp, int chunk, int mode, int pkg, const int32_t *delay_ms, const uint8_t *cohort_on, int *running, int *rc_first) {
        const int C = (int)cls_leader.size();
        int any = 0;
        for (int c = 0; c < C; c++) {
            const int g = cls_leader[(size_t)c];  // the class's one control plane
            const bool go = on(cohort_on, g) && rc_g[(size_t)g] == 0;
            for (int k = 0; k < chunk; k++) {
                Plan &pl = hp[(size_t)k * C + c];
                plan_clear(&pl);
                if (!go || rc_g[(size_t)g] != 0) continue;  // has_far = has_near = 0: both kernels skip the packet for this class's cohorts
                any = 1;
                if (mode & 1) {
                    const int r = ctl[(size_t)g].buffer_farend(pkg, &pl);
                    if (r != 0) {
                        pl.has_far = 0;
                        rc_g[(size_t)g] = r;
                        continue;
                    }
                }
                if (mode & 2) {
                    const int r = ctl[(size_t)g].process(pkg, delay_ms[g], &pl);
                    if (r != 0) {
                        plan_reject_near(&pl);
                        rc_g[(size_t)g] = r;
                    }
                }
            }
            if (go && rc_g[(size_t)g] != 0) {
                (*running)--;
                if (*rc_first == 0) *rc_first = rc_g[(size_t)g];
            }
        }
        return any;
    }
    void end_run(const uint8_t *cohort_on, int32_t *cohort_rc) const {
        if (cohort_rc)
            for (int g = 0; g < n(); g++) cohort_rc[g] = on(cohort_on, g) ? rc_g[(size_t)lead[(size_t)g]] : 0;
    }

    // ---- coalescing (wmx_*_coalesce)
    // a cohort that is restarted, retired or overwritten is no candidate of a comparison in flight
    void drop(int g) {
        for (int i = 0; i < co_n; i++)
            if (co_pairs.p[i].a == g || co_pairs.p[i].b == g) co_pairs.p[i].b = -1;
    }
    // The comparison of the pairs in flight came back (flags[i] == 1: pair i's slabs are equal).  The pairs whose planes still have
    // equal keys go to `go` with the positions of NOW (same differences, by the keys) and are reported in from / into, up to cap
    // (the rest is proposed again by a later call); the others are held off for 64 calls.  Returns the number in `go`.
    int collect(const int *flags, int32_t *from, int32_t *into, int cap, Pair *go) {
        int n_go = 0;
        for (int i = 0; i < co_n; i++) {
            Pair pc = co_pairs.p[i];
            if (pc.b < 0) continue;  // dropped by a call in between
            Key ka, kb;
            const bool ok = flags[i] == 1 && live[(size_t)pc.a] && live[(size_t)pc.b] && co_key(plane(pc.a), &ka) && co_key(plane(pc.b), &kb) &&
                            ka == kb;
            if (!ok) {
                co_retry_at[(size_t)pc.b] = co_calls + 64;
                continue;
            }
            if (n_go >= cap) continue;
            co_pair(plane(pc.a), plane(pc.b), pc.a, pc.b, &pc);
            from[n_go] = pc.b;
            into[n_go] = pc.a;
            go[n_go++] = pc;
        }
        co_n = 0;
        return n_go;
    }
    // the merged cohorts of `go` retired (co_into says where each went); returns where the id range may end now: behind the last
    // live cohort (plans, far kernel waves and the caller's per-cohort arrays are sized by it)
    int retire_merged(const Pair *go, int n_go) {
        co_into.assign((size_t)n(), -1);
        for (int i = 0; i < n_go; i++) {
            co_into[(size_t)go[i].b] = go[i].a;
            retire(go[i].b);  // its id may be handed out again
        }
        int nf = n();
        while (nf > 1 && !live[(size_t)nf - 1]) nf--;
        return nf;
    }
    void shrink(int nf) {
        ctl.resize((size_t)nf);
        lead.resize((size_t)nf);
        cls_dirty = true;
        live.resize((size_t)nf);
        co_retry_at.resize((size_t)nf);
    }
    // Up to max_pairs new pairs into co_pairs / co_n, none while a far-end group stride is in use.  Candidates: the first live cohort
    // with a key leads, every later one with the same key may join it (the lowest ids survive, so that the id range can shrink behind
    // them); keys meet through a hash of their words.  Returns the number proposed.
    int propose(int max_pairs) {
        if (max_pairs == 0 || last_far_group_stride != 0) return 0;
        if (max_pairs > kCoMax) max_pairs = kCoMax;
        std::unordered_multimap<uint64_t, int> leads;
        leads.reserve((size_t)n());
        int k = 0;
        for (int g = 0; g < n() && k < max_pairs; g++) {
            if (!live[(size_t)g]) continue;
            Key kg, kl;
            if (!co_key(plane(g), &kg)) continue;
            uint64_t hash = 1469598103934665603ull;
            for (int v : kg.v) hash = (hash ^ (uint32_t)v) * 1099511628211ull;
            int l = -1;
            const auto range = leads.equal_range(hash);
            for (auto it = range.first; it != range.second && l < 0; ++it)
                if (co_key(plane(it->second), &kl) && kl == kg) l = it->second;
            if (l < 0) {
                leads.emplace(hash, g);
                continue;
            }
            if (co_retry_at[(size_t)g] > co_calls) continue;
            co_pair(plane(l), plane(g), l, g, &co_pairs.p[k++]);
        }
        co_n = k;
        return k;
    }
};

}  // namespace wmx
