// host_ctl_san.cpp -- everything of libwmix_amd.so that decides on the HOST where data goes, compiled without HIP under
// AddressSanitizer + UndefinedBehaviorSanitizer (-fno-sanitize-recover: a finding aborts) and driven over its argument
// ranges, with the invariants the kernels rely on asserted on every plan:
//   aec_ctl.h        AecCtl:  start-up machine, delay filter, ring indices, block counters (echo_cancellation.c:599-872)
//   aecm_ctl.h       AecmCtl: the same for the AECM (echo_control_mobile.c:233-720, aecm_core.c:569-664)
//   cohort_reg.h     the cohort registry both cancellers run: ids, control-plane classes, the planning loop of a launch
//   agc_gain_table.h the gain-table recipe (digital_agc.c:61-257) for every compression gain, limiter on and off
//   mix_sched.h      zoom / load schedules and the len_of_* walks for every rate and channel pair the daemon can meet
// VERDICT r02 item 6 / SURVEY section 5.  Run by tools_dev/sanitize_cpu.sh and tests/test_sanitizers.py.
#include <cstdio>
#include <cstdlib>
#include "aec_ctl.h"
#include "aecm_ctl.h"
#include "cohort_reg.h"
#include "agc_gain_table.h"
#include "mix_sched.h"

#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) {                                                           \
            std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #c); \
            std::abort();                                                     \
        }                                                                     \
    } while (0)

using namespace wmx;

static uint32_t rng_state = 12345;
static uint32_t rnd() { return rng_state = rng_state * 1664525u + 1013904223u; }

static long drive_aec(int freq, int pkg, int mode_delay) {
    AecCtl c;
    c.init(freq);
    long blocks = 0;
    for (int p = 0; p < 6000; p++) {
        AecPlan pl;
        std::memset(&pl, 0, sizeof(pl));
        // delays: constant 0 (the daemon), constant 120, a random walk, and now and then one the reference rejects
        int d = mode_delay == 0 ? 0 : (mode_delay == 1 ? 120 : (int)(rnd() % 400));
        if (mode_delay == 3 && p % 97 == 13) d = (p & 1) ? 900 : -5;
        if (mode_delay == 3 && (rnd() % 7) == 0) continue;  // a far-end packet that never comes / a call that is skipped
        CHECK(c.buffer_farend(pkg, &pl) == 0);
        CHECK(pl.n_part >= 0 && pl.n_part <= 4 && pl.pre_wr >= 0 && pl.pre_wr < kAecPreLen && pl.far_n == pkg);
        for (int q = 0; q < pl.n_part; q++)
            CHECK(pl.part[q].pre_rd >= 0 && pl.part[q].pre_rd < kAecPreLen && pl.part[q].far_slot >= 0 && pl.part[q].far_slot < kAecFarBlocks);
        const int r = c.process(pkg, d, &pl);
        CHECK(r == 0 || r == -1);
        CHECK((d < 0 || d > 500) == (r == -1));
        if (pl.passthrough) continue;
        CHECK(pl.n_sub == pkg / kAecFrame && pl.n_blk >= 0 && pl.n_blk <= 4);
        int nb = 0;
        for (int s = 0; s < pl.n_sub; s++) {
            const AecSubPlan &sp = pl.sub[s];
            CHECK(sp.near_wr >= 0 && sp.near_wr < kAecRing && sp.out_rd >= 0 && sp.out_rd < kAecRing && sp.first_blk == nb);
            nb += sp.n_blocks;
        }
        CHECK(nb == pl.n_blk);
        for (int k = 0; k < pl.n_blk; k++) {
            const AecBlkPlan &b = pl.blk[k];
            CHECK(b.near_rd >= 0 && b.near_rd < kAecRing && b.out_wr >= 0 && b.out_wr < kAecRing);
            CHECK(b.far_slot >= 0 && b.far_slot < kAecFarBlocks && b.hist_n == blocks + k);
        }
        blocks += pl.n_blk;
        CHECK(c.blocks == (uint32_t)blocks);
    }
    return blocks;
}

static long drive_aecm(int freq, int pkg, int mode_delay) {
    AecmCtl c;
    c.init(freq);
    long blocks = 0;
    for (int p = 0; p < 6000; p++) {
        AecmPlan pl;
        std::memset(&pl, 0, sizeof(pl));
        int d = mode_delay == 0 ? 0 : (mode_delay == 1 ? 120 : (int)(rnd() % 400));
        if (mode_delay == 3 && p % 97 == 13) d = (p & 1) ? 900 : -5;
        if (mode_delay == 3 && (rnd() % 7) == 0) continue;
        CHECK(c.buffer_farend(pkg, &pl) == 0);
        CHECK(pl.far_w >= 0 && pl.far_w < kAecmFarRing && pl.far_n >= 0 && pl.far_n <= pkg);
        const int r = c.process(pkg, d, &pl);
        CHECK((d < 0 || d > 500) == (r == -1));
        if (pl.passthrough) continue;
        CHECK(pl.n_frames == pkg / kAecmFrame);
        for (int f = 0; f < pl.n_frames; f++) {
            const AecmFramePlan &fp = pl.fr[f];
            CHECK(fp.far_src >= -1 && fp.far_src < kAecmFarRing && (fp.old_slot == 0 || fp.old_slot == 1));
            CHECK(fp.ring_w >= 0 && fp.ring_w < kAecmFrameRing && fp.out_r >= 0 && fp.out_r < kAecmFrameRing && fp.n_blocks >= 0 && fp.n_blocks <= 2);
            for (int b = 0; b < fp.n_blocks; b++) {
                CHECK(fp.blk_r[b] >= 0 && fp.blk_r[b] < kAecmFrameRing && fp.blk_out_w[b] >= 0 && fp.blk_out_w[b] < kAecmFrameRing);
                CHECK(fp.blk_t[b] == blocks++);
            }
        }
    }
    return blocks;
}


// b's plan is a's under the rotations of co_pair (wmx_aec_coalesce)
static void check_rotated(const AecPlan &pa, const AecPlan &pb, const AecPairCheck &pc) {
    CHECK(pa.has_far == pb.has_far && pa.far_n == pb.far_n && pa.n_part == pb.n_part && pa.has_near == pb.has_near);
    CHECK(pa.passthrough == pb.passthrough && pa.n_sub == pb.n_sub && pa.n_blk == pb.n_blk);
    CHECK(pb.pre_wr == (pa.pre_wr + pc.d_pre) % kAecPreLen);
    for (int q = 0; q < pa.n_part; q++) {
        CHECK(pb.part[q].pre_rd == (pa.part[q].pre_rd + pc.d_pre) % kAecPreLen);
        CHECK(pb.part[q].far_slot == (pa.part[q].far_slot + pc.d_far) % kAecFarBlocks);
    }
    for (int q = 0; q < pa.n_sub; q++) {
        CHECK(pa.sub[q].near_wr == (pb.sub[q].near_wr + pc.d_near) % kAecRing && pa.sub[q].out_rd == (pb.sub[q].out_rd + pc.d_out) % kAecRing);
        CHECK(pa.sub[q].n_blocks == pb.sub[q].n_blocks && pa.sub[q].first_blk == pb.sub[q].first_blk);
    }
    for (int q = 0; q < pa.n_blk; q++) {
        CHECK(pa.blk[q].near_rd == (pb.blk[q].near_rd + pc.d_near) % kAecRing && pa.blk[q].out_wr == (pb.blk[q].out_wr + pc.d_out) % kAecRing);
        CHECK(pb.blk[q].far_slot == (pa.blk[q].far_slot + pc.d_far) % kAecFarBlocks);
        CHECK(((pb.blk[q].hist_n - pa.blk[q].hist_n - pc.d_hist) & (kAecHist - 1)) == 0);
    }
}
// the same for the AECM's plane (wmx_aecm_coalesce)
static void check_rotated(const AecmPlan &pa, const AecmPlan &pb, const AecmPairCheck &pc) {
    CHECK(pa.has_far == pb.has_far && pa.far_n == pb.far_n && pa.has_near == pb.has_near && pa.passthrough == pb.passthrough);
    CHECK(pa.n_frames == pb.n_frames && pa.discard_out == pb.discard_out);
    CHECK(pb.far_w == (pa.far_w + pc.d_ring) % kAecmFarRing);
    for (int f = 0; f < pa.n_frames && !pa.passthrough; f++) {
        const AecmFramePlan &fa = pa.fr[f], &fb = pb.fr[f];
        CHECK((fa.far_src < 0) == (fb.far_src < 0) && fa.old_slot == fb.old_slot && fa.n_blocks == fb.n_blocks);
        if (fa.far_src >= 0) CHECK(fb.far_src == (fa.far_src + pc.d_ring) % kAecmFarRing);
        CHECK(fb.ring_w == (fa.ring_w + pc.d_frame) % kAecmFrameRing && fb.out_r == (fa.out_r + pc.d_out) % kAecmFrameRing);
        for (int q = 0; q < fa.n_blocks; q++) {
            CHECK(fb.blk_r[q] == (fa.blk_r[q] + pc.d_frame) % kAecmFrameRing && fb.blk_out_w[q] == (fa.blk_out_w[q] + pc.d_out) % kAecmFrameRing);
            CHECK(((fb.blk_t[q] - fa.blk_t[q] - pc.d_hist) & (kAecmHist - 1)) == 0);
        }
    }
}

// wmx_*_coalesce's host half: two control planes started `lag` packets apart and called with the same delays.  Once their keys
// (co_key) are equal, every later plan of the younger one must be the older one's plan under the rotations of co_pair --
// for thousands of packets, with the delay changing on the way at packet `step` (both see the same change).  Returns the packet at
// which the keys first met, or -1 if they never did.  The AECM's plane has no periodic counters, so planes meet as soon as both are
// past their start-up with the same phase of the 80-in-64 re-blocking (4 frames: 2 packets at 16 kHz, 4 at 8 kHz).
template <class Ctl>
static int drive_pair(int freq, int pkg, int lag, int delay0, int packets, int step) {
    Ctl a, b;
    a.init(freq);
    b.init(freq);
    int met = -1;
    typename Ctl::Pair pc{};
    for (int p = 0; p < packets; p++) {
        const int d = p < step ? delay0 : delay0 + 60;  // a step in the reported delay: EstBufDelay moves both planes alike
        typename Ctl::Plan pa, pb;
        std::memset(&pa, 0, sizeof(pa));
        std::memset(&pb, 0, sizeof(pb));
        CHECK(a.buffer_farend(pkg, &pa) == 0);
        CHECK(a.process(pkg, d, &pa) == 0);
        if (p < lag) continue;
        CHECK(b.buffer_farend(pkg, &pb) == 0);
        CHECK(b.process(pkg, d, &pb) == 0);
        typename Ctl::Key ka, kb;
        if (met >= 0) {
            check_rotated(pa, pb, pc);
            CHECK(co_key(a, &ka) && co_key(b, &kb) && ka == kb);  // and the keys stay equal
        } else if (co_key(a, &ka) && co_key(b, &kb) && ka == kb) {
            met = p;
            co_pair(a, b, 0, 1, &pc);
        }
    }
    return met;
}
static int drive_pair(int freq, int pkg, int lag, int delay0) { return drive_pair<AecCtl>(freq, pkg, lag, delay0, 5200, 3600); }
static int drive_pair_aecm(int freq, int pkg, int lag, int delay0) { return drive_pair<AecmCtl>(freq, pkg, lag, delay0, 4000, 2500); }

// ---- control-plane classes against a model that keeps one plane per cohort: the registry of aec.hip / aecm.hip (cohort_reg.h) runs
//      ONE plane per class and hands every member its plan.  Random histories -- cohorts added, retired, restarted, imported over,
//      switched off for a while, reporting delays of their own for a while -- and after every launch the plan a member gets through its
//      class must be the plan its own plane makes.
template <class Pair>
struct PairList {  // the modules' lists are their comparison kernels' argument
    Pair p[32];
};
template <class Ctl>
static void drive_classes(int freq, int pkg, uint32_t seed, int n_start, int ticks) {
    using Plan = typename Ctl::Plan;
    rng_state = seed;
    CohortReg<Ctl, PairList<typename Ctl::Pair>> h;
    h.init(n_start, freq);  // wmx_*_create: made together, one class
    std::vector<Ctl> model((size_t)n_start);  // the reference's way: every cohort (handle) its own plane
    for (Ctl &c : model) c.init(freq);
    std::vector<int32_t> delay, rc;
    std::vector<uint8_t> on;
    std::vector<int> odd_until((size_t)n_start, 0), off_until((size_t)n_start, 0);
    long shared = 0, launches = 0;
    for (int t = 0; t < ticks; t++) {
        // churn between launches
        const uint32_t r = rnd() % 400;  // something happens every fifth tick or so: classes have time to exist
        if (r < 4 && h.n() < 48) {  // wmx_*_add_cohort
            const int id = h.take_id();
            if (id == (int)model.size()) model.emplace_back();
            h.restart(id);
            model[(size_t)id].init(freq);
            odd_until.resize((size_t)h.n(), 0);
            off_until.resize((size_t)h.n(), 0);
        } else if (r < 7) {  // retire one
            const int g = (int)(rnd() % (uint32_t)h.n());
            if (h.live[(size_t)g] && g != 0) h.retire(g);
        } else if (r < 10) {  // restart one (aec_release + aec_init of every member)
            const int g = (int)(rnd() % (uint32_t)h.n());
            if (h.live[(size_t)g]) {
                h.restart(g);
                model[(size_t)g].init(freq);
            }
        } else if (r < 12) {  // import a cohort's plane over another (wmx_*_import_cohort)
            const int a = (int)(rnd() % (uint32_t)h.n()), b = (int)(rnd() % (uint32_t)h.n());
            if (a != b && h.live[(size_t)a] && h.live[(size_t)b]) {
                h.import(b, h.plane(a));
                model[(size_t)b] = model[(size_t)a];
            }
        } else if (r < 16) {
            odd_until[rnd() % (uint32_t)h.n()] = t + 1 + (int)(rnd() % 40);  // reports a delay of its own for a while
        } else if (r < 19) {
            off_until[rnd() % (uint32_t)h.n()] = t + 1 + (int)(rnd() % 30);  // not called for a while
        }
        delay.assign((size_t)h.n(), 0);
        on.assign((size_t)h.n(), 1);
        for (int g = 0; g < h.n(); g++) {
            if (odd_until[(size_t)g] > t) delay[(size_t)g] = 40 + 20 * (g % 3);
            if (off_until[(size_t)g] > t) on[(size_t)g] = 0;
        }
        // the launch, as wmx_*_run_cohorts does it: one packet, far and near
        int rc_first = 0, running = h.begin_run(3, 0, delay.data(), on.data());
        h.split(delay.data(), on.data());
        const std::vector<int32_t> &plan_of = h.list_classes();
        h.cls_dirty = false;
        std::vector<Plan> plans(h.cls_leader.size());
        running = h.running_classes(on.data());
        h.plan_chunk(plans.data(), 1, 3, pkg, delay.data(), on.data(), &running, &rc_first);
        CHECK(rc_first == 0);  // buffer_farend and process took every packet
        for (int g = 0; g < h.n(); g++) {
            CHECK(h.lead[(size_t)g] >= 0 && h.lead[(size_t)g] < h.n() && h.lead[(size_t)h.lead[(size_t)g]] == h.lead[(size_t)g]);  // leaders lead themselves
            if (!h.live[(size_t)g]) {
                CHECK(h.lead[(size_t)g] == g);  // a retired cohort leads nobody and follows nobody
                continue;
            }
            CHECK(h.live[(size_t)h.lead[(size_t)g]]);
            Plan want;
            std::memset(&want, 0, sizeof(want));
            if (on[(size_t)g]) {
                CHECK(model[(size_t)g].buffer_farend(pkg, &want) == 0);
                CHECK(model[(size_t)g].process(pkg, delay[(size_t)g], &want) == 0);
            }
            CHECK(std::memcmp(&want, &plans[(size_t)plan_of[(size_t)g]], sizeof(Plan)) == 0);
            CHECK(h.plane(g).same_as(model[(size_t)g]));
            shared += h.lead[(size_t)g] != g;
        }
        rc.assign((size_t)h.n(), 1);
        h.end_run(on.data(), rc.data());
        for (int32_t v : rc) CHECK(v == 0);
        launches++;
    }
    CHECK(shared > launches / 4);  // the histories do leave cohorts in shared classes (0.7 - 1 follower per launch on average here)
}

int main() {
    long total = 0;
    for (int freq : {8000, 16000})
        for (int ms : {10, 20}) {
            if (freq == 16000 && ms == 20) continue;  // 20 ms packets exist at 8 kHz only (src/webrtc.c:239-248)
            for (int md = 0; md < 4; md++) total += drive_aec(freq, freq / 1000 * ms, md) + drive_aecm(freq, freq / 1000 * ms, md);
        }
    CHECK(total > 100000);
    {
        // the comfort-noise phase table against the reference's per-draw expressions (aec_core.c:482-489) on generator states
        std::vector<AecNoiseEntry> tab((size_t)kAecNoiseTab);
        aec_noise_table(tab.data());
        uint32_t seed = 777u;
        for (int i = 0; i < 200000; i++) {
            seed = (seed * 69069u + 1u) & 0x7FFFFFFFu;
            const float r = ((float)(int16_t)(seed >> 16)) / 32768;
            const float tmp = 6.28318530717959f * r;
            CHECK((seed >> 16) < (uint32_t)kAecNoiseTab);
            CHECK(tab[seed >> 16].c == cosf(tmp) && tab[seed >> 16].s == sinf(tmp));
        }
        // the near kernel's generator: lane l's draw l (lane 0: draw 64) from the state in front of a block in ONE multiply-add, and the
        // state moved on by the 64-draw step -- against the reference's recurrence draw by draw, over 3 000 blocks from 777 and from
        // states far out
        {
            uint32_t a[65], c[65];
            for (int k = 1; k <= 64; k++) aec_lcg_jump(k, &a[k], &c[k]);
            for (uint32_t start : {777u, 0x7FFFFFFFu, 0u, 123456789u}) {
                uint32_t state = start, x = start;
                for (int blk = 0; blk < 3000; blk++) {
                    for (int k = 1; k <= 64; k++) {
                        x = (x * 69069u + 1u) & 0x7FFFFFFFu;
                        CHECK(((state * a[k] + c[k]) & 0x7FFFFFFFu) == x);
                    }
                    state = (state * a[64] + c[64]) & 0x7FFFFFFFu;
                    CHECK(state == x);
                }
            }
        }
        // k draws in one step, any start
        for (int k = 1; k <= 64; k++) {
            uint32_t a, c, s = 12345u, want = 12345u;
            aec_lcg_jump(k, &a, &c);
            for (int i = 0; i < k; i++) want = (want * 69069u + 1u) & 0x7FFFFFFFu;
            CHECK(((s * a + c) & 0x7FFFFFFFu) == want);
        }
    }
    for (uint32_t seed : {1u, 7u, 99u}) {
        drive_classes<AecCtl>(16000, 160, seed, 12, 3000);
        drive_classes<AecCtl>(8000, 80, seed + 1000, 5, 2500);
        drive_classes<AecCtl>(8000, 160, seed + 2000, 30, 1500);
        drive_classes<AecmCtl>(16000, 160, seed, 12, 3000);
        drive_classes<AecmCtl>(8000, 80, seed + 1000, 5, 2500);
        drive_classes<AecmCtl>(8000, 160, seed + 2000, 30, 1500);
    }
    // ---- coalescing: planes meet as soon as the younger one's start-up is over when they are a multiple of the re-blocking period
    //      apart (160-in-64: 2 packets; 80-in-64: 4 packets) -- the core's two block counters count with the stream, not with the plane
    //      -- and never when they are not (another block phase)
    for (int freq : {8000, 16000})
        for (int d0 : {0, 40, 120}) {
            const int pkg = freq / 100, period = freq == 16000 ? 2 : 4;
            for (int lag : {period, 3 * period, 104, 800}) {
                const int met = drive_pair(freq, pkg, lag, d0);
                CHECK(met >= 0 && met < lag + 400);
            }
            for (int lag : {1, period + 1, 37}) CHECK(drive_pair(freq, pkg, lag, d0) < 0);
        }
    CHECK(drive_pair(8000, 160, 2, 0) >= 0 && drive_pair(8000, 160, 3, 0) < 0);  // 20 ms packets at 8 kHz (the daemon's cadence)
    for (int freq : {8000, 16000})
        for (int d0 : {0, 40, 120}) {
            const int pkg = freq / 100, period = freq == 16000 ? 2 : 4;
            for (int lag : {period, 3 * period, 100, 800}) CHECK(drive_pair_aecm(freq, pkg, lag, d0) >= 0);
            for (int lag : {1, period + 1, 37}) CHECK(drive_pair_aecm(freq, pkg, lag, d0) < 0);
        }
    // ---- AGC gain table: every compression gain an uint8 agc_addition() can pass, limiter off (wmix) and on
    int ok = 0;
    for (int comp = 0; comp < 256; comp++)
        for (int lim = 0; lim < 2; lim++) {
            int32_t t[32];
            const int16_t c16 = (int16_t)comp;
            if (host_gain_table(t, c16, 0, lim != 0, analog_target_for(c16)) == 0) {
                ok++;
                for (int i = 1; i < 32; i++) CHECK(t[i] >= 0);
            }
        }
    CHECK(ok > 100);
    // ---- mixer schedules: every format pair of the daemon's rates x {1, 2} channels, ragged lengths
    const int rates[] = {8000, 11025, 16000, 22050, 32000, 44100, 48000};
    size_t entries = 0;
    for (int fi : rates)
        for (int fo : rates)
            for (int ci = 1; ci <= 2; ci++)
                for (int co = 1; co <= 2; co++)
                    for (uint32_t len : {0u, 2u, 6u, 320u, 1282u, 3528u, 7680u}) {
                        std::vector<int32_t> idx;
                        zoom_schedule((uint8_t)ci, (uint16_t)fi, len, (uint8_t)co, (uint16_t)fo, idx);
                        for (int32_t v : idx) CHECK(v >= 0 && (uint32_t)v * 2u < len + 2u * (uint32_t)ci);
                        const uint32_t lo = len_walk((uint8_t)ci, (uint16_t)fi, (uint8_t)co, (uint16_t)fo, len / 2, true, false);
                        const uint32_t li = len_walk((uint8_t)ci, (uint16_t)fi, (uint8_t)co, (uint16_t)fo, len / 2, false, true);
                        (void)lo;
                        (void)li;
                        std::vector<LoadEntry> sch;
                        if (load_schedule(co, fo, len, (uint16_t)fi, (uint8_t)ci, 16, sch))
                            for (const LoadEntry &e : sch) {
                                CHECK(e.src >= 0 && (uint32_t)e.src * 2u <= len + 4u * (uint32_t)ci);
                                CHECK(e.k >= -1 && e.k < 64 && e.n2 >= 0 && e.n2 <= 64);
                            }
                        entries += idx.size() + sch.size();
                        sch.clear();
                        load_schedule(co, fo, len, (uint16_t)fi, (uint8_t)ci, 8, sch);  // the reference's empty 8-bit branch
                        CHECK(sch.empty() || (fi == fo && ci == co));
                    }
    CHECK(entries > 100000);
    std::printf("host control planes: %ld AEC/AECM blocks planned, %d gain tables, %zu schedule entries -- clean under ASan + UBSan\n", total,
                ok, entries);
    return 0;
}
