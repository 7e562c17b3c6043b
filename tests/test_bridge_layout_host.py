"""The host logic of the bridge over a layout on the CPU (wmix_amd/csrc/bridge_layout.h): validation, the partition into the four size
classes, the carrying-over of the cursors from one layout to the next, and the plan of one load call (the cursor rule once per distinct
start value, the conferences' start columns as leads that a steady step leaves alone).  A stand-alone C++ driver against the header
mix.hip and tick.hip include, built twice with g++: plain, and with the address and undefined-behaviour sanitizers (a finding kills the
driver and fails the test).  Both are plain executables."""
import os
import subprocess

import pytest

from conftest import ROOT

DRIVER = r"""
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "bridge_layout.h"

using namespace wmx;

static int failures = 0;
#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            fprintf(stderr, "line %d: %s\n", __LINE__, #cond);           \
            failures++;                                                  \
        }                                                                \
    } while (0)

static const char *build(BridgeLayout &l, int n_groups, const std::vector<std::vector<int32_t>> &confs) {
    std::vector<int32_t> off(1, 0), mem;
    for (const auto &c : confs) {
        mem.insert(mem.end(), c.begin(), c.end());
        off.push_back((int32_t)mem.size());
    }
    return bridge_layout_build(l, n_groups, (int)confs.size(), off.data(), mem.data());
}

static bool same(const BridgeLayout &a, const BridgeLayout &b) {
    return a.n_conf == b.n_conf && a.off == b.off && a.members == b.members && a.order == b.order && a.slot_of == b.slot_of && a.tab == b.tab &&
           !memcmp(a.class_begin, b.class_begin, sizeof(a.class_begin));
}

static void refusals() {
    BridgeLayout keep;
    CHECK(build(keep, 40, {{3, 1}, {7, 5, 9}}) == nullptr);
    BridgeLayout l = keep;
    std::vector<int32_t> big;
    for (int i = 0; i < 33; i++) big.push_back(i);
    CHECK(build(l, 40, {{36, 37}, big}) != nullptr && same(l, keep));         // 33 members
    big.pop_back();
    CHECK(build(l, 40, {big}) == nullptr && l.size(0) == 32);                 // 32 are fine
    l = keep;
    CHECK(build(l, 40, {{0, 40}}) != nullptr && same(l, keep));               // a ring index outside [0, n_groups)
    CHECK(build(l, 40, {{0, -1}}) != nullptr && same(l, keep));
    CHECK(build(l, 40, {{0, 1, 0}}) != nullptr && same(l, keep));             // a ring twice in one conference
    CHECK(build(l, 40, {{0, 1}, {2, 1}}) != nullptr && same(l, keep));        // ... and in two
    CHECK(build(l, 40, {{4}, {4}}) != nullptr && same(l, keep));              // placeholders are members too
    const int32_t off_back[] = {0, 3, 2, 4}, off_late[] = {1, 2, 4}, mem[] = {0, 1, 2, 3};
    CHECK(bridge_layout_build(l, 40, 3, off_back, mem) != nullptr && same(l, keep));  // the offsets do not ascend
    CHECK(bridge_layout_build(l, 40, 2, off_late, mem) != nullptr && same(l, keep));  // ... or do not start at 0
    CHECK(bridge_layout_build(l, 40, -1, off_back, mem) != nullptr && same(l, keep));
    CHECK(bridge_layout_build(l, 40, 2, nullptr, mem) != nullptr && same(l, keep));
    const int32_t off_ok[] = {0, 2, 4};
    CHECK(bridge_layout_build(l, 40, 2, off_ok, nullptr) != nullptr && same(l, keep));
    CHECK(bridge_layout_build(l, 40, 0, nullptr, nullptr) == nullptr && l.n_conf == 0 && l.slots() == 0);  // n_conf == 0 clears
}

static void classes() {
    const int sizes[] = {0, 1, 2, 4, 5, 8, 9, 16, 17, 32}, want[] = {-1, -1, 0, 0, 1, 1, 2, 2, 3, 3};
    for (int k = 0; k < 10; k++) CHECK(bridge_size_class(sizes[k]) == want[k]);
    CHECK(bridge_size_class(33) == -1 && bridge_size_class(-3) == -1);
    for (int k = 0; k < kBridgeClasses; k++) CHECK(bridge_class_bound(k) == (4 << k));
    // a layout of those sizes, largest first, members descending: 94 rings
    std::vector<std::vector<int32_t>> confs;
    int32_t next = 93;
    for (int k = 9; k >= 0; k--) {
        confs.emplace_back();
        for (int i = 0; i < sizes[k]; i++) confs.back().push_back(next--);
    }
    CHECK(next == -1);
    BridgeLayout l;
    CHECK(build(l, 94, confs) == nullptr);
    CHECK(l.slots() == 8);
    const int begin[] = {0, 2, 4, 6, 8};
    for (int k = 0; k <= kBridgeClasses; k++) CHECK(l.class_begin[k] == begin[k]);
    // conference index = 9 - k; inside a class the index order is kept
    const int order[] = {6, 7, 4, 5, 2, 3, 0, 1};
    for (int s = 0; s < 8; s++) {
        const int c = order[s];
        CHECK(l.order[s] == c && l.slot_of[c] == s && l.tab[2 * s] == l.off[c] && l.tab[2 * s + 1] == l.size(c));
        CHECK(l.size(c) <= bridge_class_bound(s / 2) && (s / 2 == 0 || l.size(c) > bridge_class_bound(s / 2 - 1)));
    }
    CHECK(l.slot_of[8] == -1 && l.slot_of[9] == -1 && l.size(8) == 1 && l.size(9) == 0);
}

struct Run {  // what wmx_tick keeps: the layout's sizes and one cursor per conference index
    BridgeLayout l;
    std::vector<int32_t> sizes;
    std::vector<uint32_t> head, tick, next;
    BridgeLeads leads;
    void layout(int n_groups, const std::vector<std::vector<int32_t>> &confs) {
        CHECK(build(l, n_groups, confs) == nullptr);
        leads.valid = false;  // wmx_mix_set_conferences
        bridge_cursors_carry(sizes, l, head, tick);
        sizes.clear();
        for (int c = 0; c < l.n_conf; c++) sizes.push_back(l.size(c));
    }
    BridgePlan load(const BridgeMixState &m, uint32_t n_out) { return bridge_plan_load(l, m, n_out, head.data(), tick.data(), leads, next); }
};

// the reference's rule for one call, restated from src/wmix.c:1666-1673 and :1942-1956 for a cursor that is not behind the tick
static void reference_step(const BridgeMixState &m, uint32_t n_out, uint32_t &head, uint32_t &tick, uint32_t &start) {
    if (head == UINT32_MAX || tick < m.tick) {
        head = m.head_off + m.play_correct;
        tick = m.tick + m.play_correct;
        if (head >= m.ring_bytes) head = 0;
    }
    start = head;
    head = (head + 2 * n_out) % m.ring_bytes;
    tick += 2 * n_out;
}

static void cursors() {
    // 1 x 8000 ring, platform/alsa's 3 200 bytes, 160-sample packages; the play thread drains one package before every load
    BridgeMixState m{0, 0, 3200, 16000};
    const uint32_t N = 160;
    Run r;
    uint32_t want_h[3] = {UINT32_MAX, UINT32_MAX, UINT32_MAX}, want_t[3] = {0, 0, 0}, start[3] = {0, 0, 0};
    int uploads = 0, steady_uploads = 0;
    bool differed = false;
    std::vector<std::vector<int32_t>> confs;
    for (int t = 0; t < 130; t++) {
        bool changed = true;
        if (t == 0) confs = {{0, 1}, {2, 3, 4}};
        else if (t == 40) confs = {{0, 1, 5}, {2, 3, 4}};               // a leg joins: conference 0 keeps its cursor
        else if (t == 45) confs = {{0, 1, 5}, {2, 3, 4}, {6, 7, 8}};    // one forms: fresh
        else if (t == 60) confs = {{0, 1, 5}, {2, 4}, {6, 7, 8}};       // a leg leaves: kept
        else if (t == 80) confs = {{0, 1, 5}, {2}, {6, 7, 8}};          // down to one: forgotten
        else if (t == 100) confs = {{0, 1, 5}, {2, 4}, {6, 7, 8}};      // re-forms: fresh
        else changed = false;
        if (changed) {
            r.layout(10, confs);
            for (size_t c = 0; c < confs.size(); c++)
                if (confs[c].size() < 2) want_h[c] = UINT32_MAX, want_t[c] = 0;
        }
        m.head_off = (m.head_off + 2 * N) % m.ring_bytes;
        m.tick += 2 * N;
        for (size_t c = 0; c < confs.size(); c++)
            if (confs[c].size() >= 2) reference_step(m, N, want_h[c], want_t[c], start[c]);
        const std::vector<uint32_t> before = r.leads.lead;
        const BridgePlan plan = r.load(m, N);
        uploads += plan.upload;
        if (!changed) steady_uploads += plan.upload;
        CHECK(plan.upload == (changed || before != r.leads.lead));
        for (size_t c = 0; c < confs.size(); c++) {
            CHECK(r.head[c] == want_h[c] && r.tick[c] == want_t[c]);
            const int s = r.l.slot_of[c];
            if (s >= 0) CHECK((plan.base_sample + r.leads.lead[(size_t)s]) % 8000 == start[c] / 2);
        }
        if (t == 45) {
            // the head stands at 46 * 320 = 14 720 > 16 000 - 3 200: the fresh cursor of conference 2 is the ring's start, while
            // conference 0's, begun at tick 0, runs 3 200 bytes in front of the head
            CHECK(start[2] == 0 && start[0] == (14720 + 3200) % 16000 && plan.distinct == 2);
        }
        if (t > 45) differed = differed || r.head[0] != r.head[2];
        if (t == 79) CHECK(r.head[1] != UINT32_MAX);
        if (t >= 80 && t < 100) CHECK(r.head[1] == UINT32_MAX && r.tick[1] == 0);
        if (t == 100) CHECK(start[1] == (101 * 320 + 3200) % 16000);
    }
    CHECK(differed);             // two conferences alive together at different ring positions, for good
    CHECK(steady_uploads == 0);  // a steady step requests no lead upload
    CHECK(uploads == 6);         // one per layout
    // a mixer nobody drains (wmx_mix_load_minus_conf on its own): cursors that advance alike leave the leads alone too
    Run q;
    q.layout(6, {{0, 1}, {2, 3, 4}});
    BridgeMixState still{640, 0, 3200, 16000};
    CHECK(q.load(still, N).upload);
    for (int k = 0; k < 60; k++) CHECK(!q.load(still, N).upload);  // across the ring's end as well
    q.head[1] = UINT32_MAX;                                           // one re-forms while the other goes on
    const BridgePlan p = q.load(still, N);
    CHECK(p.upload && p.distinct == 2 && q.head[0] != q.head[1]);
    CHECK(!q.load(still, N).upload);
    // more distinct start values than are remembered: still every conference's own
    std::vector<std::vector<int32_t>> many;
    for (int32_t c = 0; c < 12; c++) many.push_back({2 * c, 2 * c + 1});
    Run w;
    w.layout(24, many);
    for (uint32_t c = 0; c < 12; c++) w.head[c] = 320 * c, w.tick[c] = 5000 + c;
    w.load(still, N);
    for (uint32_t c = 0; c < 12; c++) {
        CHECK(w.head[c] == 320 * c + 320 && w.tick[c] == 5000 + c + 320);
        CHECK((w.leads.lead[c] + 8000 - w.leads.lead[0]) % 8000 == 160 * c);
    }
    // carrying over into a shorter and a longer layout
    w.layout(24, {{0, 1}});
    CHECK(w.head.size() == 1 && w.head[0] == 320);
    w.layout(24, {{0, 1}, {}, {4, 5}});
    CHECK(w.head.size() == 3 && w.head[0] == 320 && w.head[1] == UINT32_MAX && w.head[2] == UINT32_MAX);
}

int main() {
    refusals();
    classes();
    cursors();
    printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
"""


@pytest.fixture(scope="module")
def driver_source(tmp_path_factory):
    src = tmp_path_factory.mktemp("bridge_layout") / "bridge_layout_driver.cpp"
    src.write_text(DRIVER)
    return src


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]],
                         ids=["plain", "sanitized"])
def test_bridge_layout_header(driver_source, flags):
    exe = driver_source.with_name("driver_" + ("san" if len(flags) > 1 else "plain"))
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function"] + flags +
                          ["-I" + os.path.join(ROOT, "wmix_amd", "csrc"), "-o", str(exe), str(driver_source)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "0 failures" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
