// feed_state.h -- which way a graph's change feed polls next (rf_graph_feed_*,
// DESIGN.md §5 "Change feed").
//
// A poll finds the job-output slots whose digests moved since the last poll.
// After exactly one plain incremental step the jobs that can have moved are
// known: that step's level lists, and the slot-fused jobs of the input slots
// marked for it (recorded as they were marked).  The poll then compares those
// candidates only (LISTED).  Anything else that wrote slots or lists since the
// last poll -- a second step, a full recompute, an adopted table, a captured
// step, input slots set after the step (the mark kernels hash slot-fused
// chains at once and append to the lists the step left) -- leaves the lists
// short of the whole story, and the poll compares every tracked slot (SCAN).
//
// A pure function of its arguments: no HIP, no clocks, no environment.
#pragma once
#include <stdint.h>

namespace rf {

// (the values of RF_FEED_NONE / RF_FEED_LISTED / RF_FEED_SCAN, reflow_hip.h)
enum FeedMode : uint32_t { kFeedNone = 0, kFeedListed = 1, kFeedScan = 2 };

enum FeedEvent : uint32_t {
    kFeedOpen = 0,      // rf_graph_feed_open: the baseline is the table as it stands
    kFeedSetSlots,      // input slots marked on the recomputed graph (set_slots, set_slots_device, update)
    kFeedPlainStep,     // a whole plain incremental step was queued
    kFeedFull,          // a full recompute
    kFeedOtherWrite,    // any other slot write: adopt, a captured-graph step, a partial step
    kFeedPoll,          // a poll ran (its mode: feed_next_mode before this event)
    kFeedEventCount
};

// What has happened since the last poll (or the open).
enum FeedPhase : uint32_t {
    kFeedClean = 0,  // nothing
    kFeedMarked,     // input slots set, no step yet
    kFeedStepped,    // zero or more set_slots, then exactly one plain step, nothing after it
    kFeedDirty       // anything else
};

struct FeedState {
    FeedPhase phase = kFeedClean;
};

// The mode of a poll run now, and whether a LISTED poll has candidates (the
// last step's lists and the recorded slot-fused jobs) or only what earlier
// polls left pending.
struct FeedPlan {
    FeedMode mode;
    bool candidates;
};
FeedPlan feed_next_mode(const FeedState& s, bool force_scan);

// Whether the slot-fused jobs of input slots marked now belong to the next
// LISTED poll's candidates (so the caller records them): before the event is
// applied.
bool feed_records_marks(const FeedState& s);

void feed_apply(FeedState& s, FeedEvent e);

}  // namespace rf
