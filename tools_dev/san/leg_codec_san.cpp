// leg_codec_san.cpp -- the codec rule of an RTP leg (wmix_amd/csrc/leg_codec.h) as a stand-alone CPU program, for AddressSanitizer +
// UndefinedBehaviorSanitizer (tests/test_leg_codec_host.py compiles it with g++).  No HIP, no GPU.
//
//   leg_codec_san         every case: 4 codecs x arrived / not arrived x 128 payload types, one result line per case in that order:
//                         in_codec arrived pt call ulaw refused
//                         then one line per law: "law" out_law payload-type, and one per value -1 .. 4: "valid" v codec? law?
#include <cstdint>
#include <cstdio>
#include "leg_codec.h"

using namespace wmx;

int main() {
    long bad = 0;
    for (uint32_t codec = 0; codec < 4; codec++)
        for (int arrived = 0; arrived < 2; arrived++)
            for (uint32_t pt = 0; pt < 128; pt++) {
                const uint32_t r = leg_codec_slot(arrived != 0, pt, codec);
                const int call = (r & kLegCodecCall) != 0u, ulaw = (r & kLegCodecUlaw) != 0u, refused = (r & kLegCodecRefused) != 0u;
                printf("%u %d %u %d %d %d\n", codec, arrived, pt, call, ulaw, refused);
                // what every answer satisfies: no other bit, a law only for a call, refused exactly when something arrived that is no call
                if ((r & ~7u) || (ulaw && !call) || refused != (arrived && !call)) bad++;
            }
    for (int law = 0; law < 2; law++) printf("law %d %u\n", law, leg_codec_out_pt(law));
    for (int v = -1; v <= 4; v++) printf("valid %d %d %d\n", v, (int)leg_codec_valid(v), (int)leg_law_valid(v));
    if (bad) fprintf(stderr, "%ld cases break what every answer satisfies\n", bad);
    return bad ? 1 : 0;
}
