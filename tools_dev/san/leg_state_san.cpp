// leg_state_san.cpp -- where the columns of a per-leg state table lie (LegLayout, wmix_amd/csrc/leg_state.h) as a stand-alone CPU program,
// for AddressSanitizer + UndefinedBehaviorSanitizer (tools_dev/san/Makefile).  No HIP, no GPU.
//
//   leg_state_san         every table at every leg count 1 .. 17, the count innermost
// First the bridge's eight tables as the handles construct them -- the header's own lists: senders, sequence, codec (sent law 1),
// concealment, DTMF, cursors, talkers, gate --, then four that break the layout rule.  Per table and leg count one line
//   T <table> <n_legs> <n_cols> <aligned>
// and per column c one line
//   C <bytes> <fill> <offset> <run_end any width> <run_end same width>     (both runs up to the table's end)
// and behind the columns the block's size
//   S <offset(n_cols)>
// Every case also checks what any layout satisfies; a violation is counted and fails the run.
#include <cstdio>
#include "leg_state.h"

using namespace wmx;

int main() {
    const LegColumns tables[] = {
        kLegSendColumns, kLegSeqColumns, leg_codec_columns(kLawU), kLegPlcColumns, kLegDtmfColumns, kLegCursorColumns, kLegTalkerColumns,
        kLegGateColumns,
        // broken: a byte in front of a word; a half-word that leaves a word off its grid; 12 bytes in front of 16; a word in front of 8 bytes
        LegColumns{{{1, 0}, {4, 0}}},
        LegColumns{{{4, 0}, {2, 0}, {4, 0}}},
        LegColumns{{{12, 0}, {16, 0}}},
        LegColumns{{{8, 0}, {4, 0}, {8, 0}}},
    };
    long bad = 0;
    int t = 0;
    for (const LegColumns &cols : tables) {
        for (int n = 1; n <= 17; n++) {
            const LegLayout l(n, cols);
            printf("T %d %d %d %d\n", t, n, l.n_cols, l.aligned ? 1 : 0);
            for (int c = 0; c < l.n_cols; c++) {
                const int any = l.run_end(c, false, l.n_cols), same = l.run_end(c, true, l.n_cols);
                printf("C %zu %d %zu %d %d\n", l.col[c].bytes, l.col[c].fill, l.offset(c), any, same);
                // a run is not empty, ends inside the table, and one width more never makes it longer; an aligned table hands out
                // no entry off its alignment
                if (same <= c || same > any || any > l.n_cols) bad++;
                if (l.aligned && l.offset(c) % LegLayout::alignment(l.col[c].bytes) != 0) bad++;
            }
            printf("S %zu\n", l.offset(l.n_cols));
        }
        t++;
    }
    if (bad) fprintf(stderr, "%ld cases break what every layout satisfies\n", bad);
    return bad ? 1 : 0;
}
