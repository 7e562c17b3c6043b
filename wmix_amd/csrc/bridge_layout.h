// bridge_layout.h -- the host logic behind wmx_mix_set_conferences / wmx_mix_load_minus_conf (mix.hip) and
// wmx_tick_bridge_conferences (tick.hip): conferences of different sizes whose members come and go.
//
// A layout is n_conf conferences; conference c is the ordered list members[off[c] .. off[c+1]) of ring indices (the order of the
// saturating adds, mix_minus.h).  A ring is in at most one conference; a conference of 0 or 1 members is a placeholder that keeps
// its index and loads nothing.  Every conference has a cursor (head[c], tick[c]) of its own: one that forms starts from a fresh
// cursor, which by src/wmix.c:1666-1673 is head + VIEW_PLAY_CORRECT or the START of the ring when that lies behind its end, so two
// conferences alive at the same time can write at different ring positions for good.
//
// What is here: validation; the partition into the four size classes of load_minus_conf_kernel<PMAX> (a two-party call does not
// run in the 32-wide instantiation); the carrying-over of cursors from one layout to the next; and the plan of one load call -- the
// cursor rule applied once per DISTINCT start value (a handful are alive at a time, whatever the number of conferences), and every
// conference's start column as a lead relative to one launch argument, so that a steady tick (no layout change, every cursor
// advancing by the package) uploads nothing per conference.
//
// Plain C++ without HIP types: mix.hip and tick.hip include it, tests/test_bridge_layout_host.py compiles it with g++.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>
#include "mix_cursor.h"

namespace wmx {

constexpr int kBridgeMaxParties = 32;  // WMX_MIX_MAX_PARTIES (include/wmix_amd.h)
constexpr int kBridgeClasses = 4;      // conferences of <= 4, <= 8, <= 16, <= 32 members

// the size class of a conference of n members: 0 .. 3, or -1 when it loads nothing (n < 2) or is refused (n > 32)
inline int bridge_size_class(int n) {
    if (n < 2 || n > kBridgeMaxParties) return -1;
    return n <= 4 ? 0 : n <= 8 ? 1 : n <= 16 ? 2 : 3;
}
inline int bridge_class_bound(int cls) { return 4 << cls; }

struct BridgeLayout {
    int n_conf = 0;
    std::vector<int32_t> off, members;  // as the caller gave them: off has n_conf + 1 entries
    // The live conferences (>= 2 members) sorted by size class, index order inside a class: slot s is conference order[s], and class
    // k owns the slots class_begin[k] .. class_begin[k + 1].  tab holds {off, size} per slot: what the kernel reads.
    std::vector<int32_t> order, slot_of, tab;
    int class_begin[kBridgeClasses + 1] = {0, 0, 0, 0, 0};

    int size(int c) const { return c >= 0 && c < n_conf ? off[(size_t)c + 1] - off[(size_t)c] : 0; }
    int slots() const { return (int)order.size(); }
};

// Validates a caller's layout for a mixer of n_groups rings and builds `out` from it.  Returns nullptr, or what is wrong with it --
// and then `out` is untouched.
inline const char *bridge_layout_build(BridgeLayout &out, int n_groups, int n_conf, const int32_t *off, const int32_t *members) {
    if (n_conf < 0 || n_groups < 1) return "a negative number of conferences";
    if (n_conf == 0) {
        out = BridgeLayout();
        return nullptr;
    }
    if (!off) return "no offsets";
    if (off[0] != 0) return "off[0] is not 0";
    for (int c = 0; c < n_conf; c++) {
        if (off[c + 1] < off[c]) return "the offsets do not ascend";
        if (off[c + 1] - off[c] > kBridgeMaxParties) return "a conference of more than WMX_MIX_MAX_PARTIES members";
    }
    const int32_t total = off[n_conf];
    if (total > 0 && !members) return "no member list";
    std::vector<uint8_t> seen((size_t)n_groups, 0);
    for (int32_t i = 0; i < total; i++) {
        const int32_t r = members[i];
        if (r < 0 || r >= n_groups) return "a ring index outside the mixer";
        if (seen[(size_t)r]) return "a ring listed twice";
        seen[(size_t)r] = 1;
    }
    BridgeLayout l;
    l.n_conf = n_conf;
    l.off.assign(off, off + n_conf + 1);
    l.members.assign(members, members + total);
    l.slot_of.assign((size_t)n_conf, -1);
    for (int k = 0; k < kBridgeClasses; k++) {
        l.class_begin[k] = (int)l.order.size();
        for (int c = 0; c < n_conf; c++)
            if (bridge_size_class(l.size(c)) == k) {
                l.slot_of[(size_t)c] = (int32_t)l.order.size();
                l.order.push_back(c);
                l.tab.push_back(l.off[(size_t)c]);
                l.tab.push_back(l.size(c));
            }
    }
    l.class_begin[kBridgeClasses] = (int)l.order.size();
    out = std::move(l);
    return nullptr;
}

// The cursors from one layout to the next.  Conference identity is the index: a conference that had 2 or more members and still has
// keeps its cursor (a leg that joins is loaded from it; the legs already there hear no gap and no overlap); one that has fewer than 2
// now, or had fewer than 2 before, has none -- the next load starts it from a fresh one.
inline void bridge_cursors_carry(const std::vector<int32_t> &old_sizes, const BridgeLayout &now, std::vector<uint32_t> &head,
                                 std::vector<uint32_t> &tick) {
    head.resize((size_t)now.n_conf, UINT32_MAX);
    tick.resize((size_t)now.n_conf, 0);
    for (int c = 0; c < now.n_conf; c++) {
        const bool was = (size_t)c < old_sizes.size() && old_sizes[(size_t)c] >= 2;
        if (!was || now.size(c) < 2) head[(size_t)c] = UINT32_MAX, tick[(size_t)c] = 0;
    }
}

// One wmix_load_data call's cursor arithmetic (mix_cursor.h): where a call that is handed (head, tick) starts, and the cursor it ends
// with after n_out ring samples.
inline void bridge_cursor_step(const BridgeMixState &m, uint32_t n_out, uint32_t &head, uint32_t &tick, uint32_t &start) {
    mix_cursor_begin(m, head, tick);
    start = head;
    mix_cursor_end(m, n_out, head, tick);
}

// the leads the device holds (one per slot, in ring samples), and whether it holds any
struct BridgeLeads {
    std::vector<uint32_t> lead;
    bool valid = false;
};

struct BridgePlan {
    uint32_t base_sample = 0;  // the launch argument: slot s starts at ring sample (base_sample + lead[s]) mod the ring
    bool upload = false;       // the leads changed (or the layout did): `dev.lead` has to go to the device before the launch
    int distinct = 0;          // start values the cursor rule was applied to
};

// One load call over the layout: head[] / tick[] (n_conf entries) in and out.  A conference of fewer than 2 members forgets its cursor.
// Leads are kept relative to the first slot's start, so cursors that advance alike -- and a play head that moves or does not --
// leave them as they are.  `next` is scratch the caller keeps to spare the allocation.
inline BridgePlan bridge_plan_load(const BridgeLayout &l, const BridgeMixState &m, uint32_t n_out, uint32_t *head, uint32_t *tick,
                                   BridgeLeads &dev, std::vector<uint32_t> &next) {
    struct Seen {
        uint32_t head_in, tick_in, start, head_out, tick_out;
    };
    Seen seen[8];
    int n_seen = 0;
    BridgePlan plan;
    const uint32_t ring_samples = m.ring_bytes / 2;
    next.assign((size_t)l.slots(), 0);
    for (int c = 0; c < l.n_conf; c++) {
        const int32_t slot = l.slot_of[(size_t)c];
        if (slot < 0) {
            head[c] = UINT32_MAX, tick[c] = 0;
            continue;
        }
        const Seen *hit = nullptr;
        for (int k = 0; k < n_seen && !hit; k++)
            if (seen[k].head_in == head[c] && seen[k].tick_in == tick[c]) hit = &seen[k];
        Seen one;
        if (!hit) {
            one.head_in = one.head_out = head[c];
            one.tick_in = one.tick_out = tick[c];
            bridge_cursor_step(m, n_out, one.head_out, one.tick_out, one.start);
            plan.distinct++;
            // a handful are remembered; a start value beyond them is computed where it is met (correct, only not shared)
            if (n_seen < (int)(sizeof(seen) / sizeof(seen[0]))) seen[n_seen++] = one;
            hit = &one;
        }
        head[c] = hit->head_out, tick[c] = hit->tick_out;
        next[(size_t)slot] = (hit->start / 2) % ring_samples;
    }
    if (next.empty()) return plan;
    plan.base_sample = next[0];
    for (uint32_t &v : next) v = (v + ring_samples - plan.base_sample) % ring_samples;
    if (!dev.valid || dev.lead != next) {
        dev.lead.swap(next);
        dev.valid = true;
        plan.upload = true;
    }
    return plan;
}

}  // namespace wmx
