// leg_echo_san.cpp -- the control plane of one leg's echo canceller (AecmCtl, wmix_amd/csrc/aecm_ctl.h: the text aecm_legs_kernel runs
// per leg on the device) as a stand-alone CPU program, for AddressSanitizer + UndefinedBehaviorSanitizer (tools_dev/san/Makefile).
// No HIP, no GPU.
//
//   leg_echo_san < scripts     one script per line of stdin: the reported delay in ms, then the near rows of each tick (0 .. 4)
// Per tick the leg's rows first -- each one AecmCtl::process(160, delay) -- then the tick's far row, AecmCtl::buffer_farend(160): the
// order of wmx_aecm_process_legs.  One result line behind every call: ec_startup known_delay rd wr diff_wrap of the far ring; a line
// "end" behind every script (tests/test_leg_echo_ctl_host.py compares every line with the oracle's handle).  Every call also checks
// what any plan satisfies -- positions inside their rings, at most two blocks per frame, a far write of at most 160 samples that
// fits; a violation is counted and fails the run.  Without input: nothing but the exit code.
#include <cstdint>
#include <cstdio>
#include <sstream>
#include <string>
#include <iostream>
#include "aecm_ctl.h"

using namespace wmx;

static long bad = 0;

static void say(const AecmCtl &c) { printf("%d %d %d %d %d\n", c.ec_startup, c.known_delay, c.farend.rd, c.farend.wr, c.farend.diff_wrap); }

static void check_ring(const RingIdx &r) {
    if (r.rd < 0 || r.rd > r.count || r.wr < 0 || r.wr > r.count || r.avail_read() < 0 || r.avail_read() > r.count) bad++;
}

static void check_plan(const AecmCtl &c, const AecmPlan &pl) {
    check_ring(c.farend);
    check_ring(c.frame_ring);
    check_ring(c.out_ring);
    if (pl.has_far && (pl.far_w < 0 || pl.far_w >= kAecmFarRing || pl.far_n < 0 || pl.far_n > 160)) bad++;
    if (!pl.has_near || pl.passthrough) return;
    if (pl.n_frames != 2) bad++;
    for (int f = 0; f < pl.n_frames && f < 2; f++) {
        const AecmFramePlan &fp = pl.fr[f];
        if (fp.far_src < -1 || fp.far_src >= kAecmFarRing || fp.old_slot != f || fp.ring_w < 0 || fp.ring_w >= kAecmFrameRing) bad++;
        if (fp.n_blocks < 0 || fp.n_blocks > 2 || fp.out_r < 0 || fp.out_r >= kAecmFrameRing) bad++;
        for (int b = 0; b < fp.n_blocks && b < 2; b++)
            if (fp.blk_r[b] < 0 || fp.blk_r[b] >= kAecmFrameRing || fp.blk_out_w[b] < 0 || fp.blk_out_w[b] >= kAecmFrameRing || fp.blk_t[b] < 0) bad++;
    }
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        int delay, rows;
        if (!(in >> delay)) continue;
        // on the heap, exactly one of each: a write behind either is the sanitizer's to report
        AecmCtl *c = new AecmCtl();
        c->init(8000);
        while (in >> rows) {
            for (int r = 0; r < rows; r++) {
                AecmPlan *pl = new AecmPlan();
                plan_clear(pl);
                if (c->process(160, delay, pl) != 0) bad++;
                check_plan(*c, *pl);
                delete pl;
                say(*c);
            }
            AecmPlan *pl = new AecmPlan();
            plan_clear(pl);
            if (c->buffer_farend(160, pl) != 0) bad++;
            check_plan(*c, *pl);
            delete pl;
            say(*c);
        }
        delete c;
        printf("end\n");
    }
    if (bad) fprintf(stderr, "%ld calls break what every plan satisfies\n", bad);
    return bad ? 1 : 0;
}
