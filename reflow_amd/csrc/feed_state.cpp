// feed_state.cpp -- the change feed's poll-mode decision (feed_state.h).
#include "feed_state.h"

namespace rf {

FeedPlan feed_next_mode(const FeedState& s, bool force_scan) {
    if (force_scan) return {kFeedScan, false};
    switch (s.phase) {
        case kFeedClean: return {kFeedListed, false};   // only what earlier polls left pending
        case kFeedStepped: return {kFeedListed, true};  // the one step's lists and marks
        case kFeedMarked:  // the mark kernels already hashed the slot-fused chains
        case kFeedDirty:
        default: return {kFeedScan, false};
    }
}

bool feed_records_marks(const FeedState& s) { return s.phase == kFeedClean || s.phase == kFeedMarked; }

void feed_apply(FeedState& s, FeedEvent e) {
    switch (e) {
        case kFeedOpen:
        case kFeedPoll:  // every poll, LISTED or SCAN, leaves nothing unseen behind it
            s.phase = kFeedClean;
            return;
        case kFeedSetSlots:
            // after a step the marks write slots and lists the step's poll has not read yet
            s.phase = (s.phase == kFeedClean || s.phase == kFeedMarked) ? kFeedMarked : kFeedDirty;
            return;
        case kFeedPlainStep:
            s.phase = (s.phase == kFeedClean || s.phase == kFeedMarked) ? kFeedStepped : kFeedDirty;
            return;
        case kFeedFull:
        case kFeedOtherWrite:
        default:
            s.phase = kFeedDirty;
            return;
    }
}

}  // namespace rf
