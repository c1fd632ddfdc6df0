// feed_host_test.cpp -- the change feed through the C++ host mirror
// (include/reflow_host.hpp Eval::Feed*), on the device: after SetFileID +
// Recompute the feed reports exactly the nodes whose digests or cache keys
// moved, with the digests FlowDigest / CacheKeys read back, and the fused
// lookup equals Liveset::Contains + Assoc::GetBatch on the reported keys.
#include <cstdio>
#include <array>
#include <set>

#include "reflow_host.hpp"

using namespace reflow;

static int failures = 0;
#define EXPECT(cond, ...)                        \
    do {                                         \
        if (!(cond)) {                           \
            ++failures;                          \
            fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
            fprintf(stderr, __VA_ARGS__);        \
            fprintf(stderr, "\n");               \
        }                                        \
    } while (0)

static Fileset one(const Digest& id) {
    Fileset v;
    v.Map["."] = File{id, 0};
    return v;
}

int main() {
    try {
        Engine e(0);
        Digester D(e);
        FlowArena a;
        const Digest ida = D.FromString("a"), idb = D.FromString("b"), idc = D.FromString("c");
        // two branches; only the first reads file a
        std::vector<Flow*> outs, execs;
        for (int b = 0; b < 2; ++b) {
            Flow* va = flow::Val(a, one(b == 0 ? ida : idc));
            Flow* vb = flow::Val(a, one(idb));
            Flow* ex = flow::Exec(a, "img", "cmd %s %s # " + std::to_string(b), {va, vb});
            ex->Argmap = std::vector<ExecArg>{{false, 0}, {false, 1}, {true, 0}};
            execs.push_back(ex);
            outs.push_back(flow::Extern(a, "s3://out/" + std::to_string(b), ex));
        }
        Flow* root = flow::Merge(a, outs);
        Eval ev(e, "", /*file_slots=*/true);
        ev.Add(root);
        ev.Build();
        ev.FeedOpen();
        uint64_t found = 99;
        EXPECT(ev.FeedPoll(UINT64_MAX, false, &found).empty() && found == 0, "fresh feed reports %llu", (unsigned long long)found);
        const std::vector<Digest> keys0_before = ev.CacheKeys(execs[0]), keys1_before = ev.CacheKeys(execs[1]);
        ev.SetFileID(ida, D.FromString("a v2"));
        ev.Recompute();
        const std::vector<Eval::Changed> ch = ev.FeedPoll(UINT64_MAX, false, &found);
        EXPECT(found == ch.size() && !ch.empty(), "found %llu, written %zu", (unsigned long long)found, ch.size());
        EXPECT(ev.FeedStats().last_mode == RF_FEED_LISTED, "mode %u", ev.FeedStats().last_mode);
        std::set<std::array<uint8_t, 32>> moved;
        for (size_t i = 0; i < ch.size(); ++i) {
            EXPECT(i == 0 || ch[i - 1].slot < ch[i].slot, "slots not ascending at %zu", i);
            moved.insert(ch[i].digest.b);
        }
        // branch 0's keys and digests moved and were reported; branch 1's did not
        const std::vector<Digest> keys0 = ev.CacheKeys(execs[0]), keys1 = ev.CacheKeys(execs[1]);
        EXPECT(keys1 == keys1_before, "branch 1's cache keys moved");
        EXPECT(keys0.size() == keys0_before.size() && keys0 != keys0_before, "branch 0's cache keys did not move");
        for (const Digest& k : keys0) EXPECT(moved.count(k.b) == 1, "a moved cache key was not reported");
        for (const Digest& k : keys1) EXPECT(moved.count(k.b) == 0, "an unmoved cache key was reported");
        EXPECT(moved.count(ev.FlowDigest(root).b) == 1 && moved.count(ev.FlowDigest(outs[0]).b) == 1, "root / extern 0 not reported");
        EXPECT(moved.count(ev.FlowDigest(outs[1]).b) == 0, "extern 1 reported");
        EXPECT(ev.FeedPoll().empty(), "second poll not empty");

        // back to the old ID, through the fused lookup
        Assoc assoc(e, 64);
        Liveset live(e, 4096, 5);
        assoc.Put(AssocFileset, Digest{}, keys0_before[0], D.FromString("fsid"));
        live.Add({keys0_before[0], ev.FlowDigest(root)});
        ev.SetFileID(D.FromString("a v2"), ida);
        ev.Recompute();
        const std::vector<Eval::Looked> lk = ev.FeedLookup(&live, assoc, AssocFileset, UINT64_MAX, &found);
        EXPECT(found == lk.size() && lk.size() == ch.size(), "lookup rows %zu, want %zu", lk.size(), ch.size());
        std::vector<Digest> ks;
        for (const auto& r : lk) ks.push_back(r.key);
        const std::vector<bool> in = live.Contains(ks);
        const std::vector<std::optional<Digest>> got = assoc.GetBatch(AssocFileset, ks);
        int hits = 0;
        for (size_t i = 0; i < lk.size(); ++i) {
            EXPECT(lk[i].slot == ch[i].slot, "row %zu slot", i);
            const int want = !in[i] ? 2 : got[i] ? 1 : 0;
            EXPECT(lk[i].status == want, "row %zu status %d, want %d", i, lk[i].status, want);
            EXPECT(lk[i].value == (want == 1 ? *got[i] : Digest{}), "row %zu value", i);
            hits += want == 1;
        }
        EXPECT(hits == 1 && ev.CacheKeys(execs[0]) == keys0_before, "hits %d", hits);
        ev.FeedClose();
    } catch (const Error& err) {
        fprintf(stderr, "error %d: %s\n", err.code, err.what());
        return 2;
    }
    if (failures) return 1;
    printf("PASS\n");
    return 0;
}
