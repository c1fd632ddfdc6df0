// feed_state_test.cpp -- the change feed's poll-mode decision
// (reflow_amd/csrc/feed_state.cpp) on its own: no library, no device.
//
// Prints, for every sequence of at most 4 events after an open, one line
//   <sequence> <modes>
// sequence: '-' for the empty one, else a letter per event -- S input slots
// set, P one whole plain incremental step, F full recompute, W any other slot
// write, Q poll; modes: a letter per poll in the sequence and one for a poll
// made after it -- L listed with the step's candidates, l listed with none
// (only what earlier polls left pending), s scan.  tests/test_feed_state.py
// compares the lines with its own table.  With the argument "force" every
// poll is made with RF_FEED_FORCE_SCAN.
#include <cstdio>
#include <cstring>
#include <string>

#include "feed_state.h"

using namespace rf;

static char poll_letter(FeedState& st, bool force) {
    const FeedPlan p = feed_next_mode(st, force);
    feed_apply(st, kFeedPoll);
    if (p.mode == kFeedScan) return 's';
    if (p.mode == kFeedListed) return p.candidates ? 'L' : 'l';
    return '?';
}

static int run(const std::string& seq, bool force) {
    FeedState st;
    feed_apply(st, kFeedOpen);
    std::string modes;
    for (char c : seq) {
        switch (c) {
            case 'S':
                // marks are recorded exactly while a LISTED poll can still follow them
                feed_apply(st, kFeedSetSlots);
                break;
            case 'P': feed_apply(st, kFeedPlainStep); break;
            case 'F': feed_apply(st, kFeedFull); break;
            case 'W': feed_apply(st, kFeedOtherWrite); break;
            case 'Q': modes += poll_letter(st, force); break;
            default: return 1;
        }
    }
    FeedState after = st;
    modes += poll_letter(after, force);
    // a poll leaves nothing behind: the one after it has no candidates
    if (!force && poll_letter(after, false) != 'l') return 2;
    printf("%s %s\n", seq.empty() ? "-" : seq.c_str(), modes.c_str());
    return 0;
}

int main(int argc, char** argv) {
    const bool force = argc > 1 && !strcmp(argv[1], "force");
    const char ev[] = "SPFWQ";
    std::string seq;
    int bad = 0;
    // every sequence of length <= 4, shortest first, in the alphabet's order
    for (int len = 0; len <= 4; ++len) {
        int total = 1;
        for (int i = 0; i < len; ++i) total *= 5;
        for (int k = 0; k < total; ++k) {
            seq.assign((size_t)len, ' ');
            for (int i = len - 1, q = k; i >= 0; --i, q /= 5) seq[(size_t)i] = ev[q % 5];
            bad += run(seq, force);
        }
    }
    // marks are recorded (for the next LISTED poll) before a step only
    {
        FeedState st;
        feed_apply(st, kFeedOpen);
        if (!feed_records_marks(st)) ++bad;
        feed_apply(st, kFeedSetSlots);
        if (!feed_records_marks(st)) ++bad;
        feed_apply(st, kFeedPlainStep);
        if (feed_records_marks(st)) ++bad;
        feed_apply(st, kFeedPoll);
        if (!feed_records_marks(st)) ++bad;
        feed_apply(st, kFeedFull);
        if (feed_records_marks(st)) ++bad;
    }
    if (bad) {
        printf("FAIL %d\n", bad);
        return 1;
    }
    printf("PASS\n");
    return 0;
}
