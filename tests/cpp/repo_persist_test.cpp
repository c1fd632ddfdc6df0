// repo_persist_test.cpp -- the repository index read back through the C++ host
// mirror (include/reflow_host.hpp RepoIndex), on the device: List, CollectList
// with a GcLiveset's filter on TestGC's objects (the removed object is named,
// as file.Repository.Collect's os.Remove needs it,
// repository/file/repository.go:304-327) and with a nil liveset, Compact, and
// Save / Restore -- against a std::map kept here.  argv[1]: a directory for the
// saved file (default: the working directory).
#include <cstdio>
#include <map>
#include <random>
#include <string>
#include <utility>

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

using Map = std::map<std::array<uint8_t, 32>, int64_t>;

// every object once, and the set equal to the model
static bool same_set(const std::vector<RepoIndex::Object>& got, const Map& want) {
    Map m;
    for (const auto& o : got)
        if (!m.emplace(o.first.b, o.second).second) return false;
    return m == want;
}

static void check(RepoIndex& R, const Map& model, uint64_t tombstones, const char* what) {
    EXPECT(same_set(R.List(), model), "%s: the listed set", what);
    const rf_repo_stats s = R.Stats();
    int64_t bytes = 0;
    for (const auto& kv : model) bytes += kv.second;
    EXPECT(s.objects == model.size() && s.bytes == bytes && s.tombstones == tombstones,
           "%s: stats %llu objects %lld bytes %llu tombstones", what, (unsigned long long)s.objects,
           (long long)s.bytes, (unsigned long long)s.tombstones);
}

static Fileset files(Digester& D, std::initializer_list<std::pair<const char*, const char*>> specs) {
    Fileset v;
    for (const auto& s : specs) v.Map[s.first] = File{D.FromString(s.second), (int64_t)std::string(s.second).size()};
    return v;
}

int main(int argc, char** argv) {
    const std::string dir = argc > 1 ? argv[1] : ".";
    try {
        Engine e(0);
        Digester D(e);
        {
            // TestGC's repository: Collect removes exactly `unrooted`, and says so
            const std::vector<uint64_t> ptr{0, 1, 1};
            const std::vector<uint32_t> edges{1};
            GcLiveset L(e, ptr, edges);
            const Fileset interned = files(D, {{"a/x", "x"}, {"a/y", "y"}, {"a/z", "z"}, {"b/1", "1"}, {"b/2", "2"},
                                               {"c/xxx", "xxx"}, {"orphan", "orphan"}, {"unrooted", "unrooted"}});
            const Fileset result = files(D, {{"x", "x"}, {"y", "y"}, {"z", "z"}, {"1", "1"}, {"2", "2"},
                                             {"xxx", "xxx"}, {"anotherfile", "orphan"}});
            RepoIndex R(e);
            Map model;
            std::vector<Digest> ids;
            std::vector<int64_t> sizes;
            for (const auto& kv : interned.Map) {
                ids.push_back(kv.second.ID);
                sizes.push_back(kv.second.Size);
                model[kv.second.ID.b] = kv.second.Size;
            }
            R.Put(ids, sizes);
            check(R, model, 0, "TestGC put");
            L.SetValue(1, interned);
            L.SetValue(0, result);
            L.Collect({0});
            const std::vector<RepoIndex::Object> gone = R.CollectList(L);
            EXPECT(gone.size() == 1 && gone[0].first == D.FromString("unrooted") && gone[0].second == 8,
                   "collect list: %zu objects", gone.size());
            model.erase(D.FromString("unrooted").b);
            check(R, model, 1, "TestGC collected");
            EXPECT(R.CollectList(L).empty(), "a second collect finds nothing");
            check(R, model, 1, "TestGC collected twice");
            // a nil liveset: everything goes, every object named once
            const std::vector<RepoIndex::Object> all = R.CollectAllList();
            EXPECT(same_set(all, model), "collect all: the listed set");
            check(R, Map(), 8, "TestGC emptied");
            R.Compact();
            check(R, Map(), 0, "compacted empty");
        }
        {
            // random objects: removals, compaction, save, restore
            std::mt19937_64 rng(41);
            RepoIndex R(e);
            Map model;
            std::vector<Digest> ids;
            std::vector<int64_t> sizes;
            for (int i = 0; i < 3000; ++i) {
                ids.push_back(D.FromString("object " + std::to_string(i)));
                sizes.push_back((int64_t)(rng() % 100000));
                model[ids.back().b] = sizes.back();
            }
            R.Put(ids, sizes);
            check(R, model, 0, "random put");
            std::vector<Digest> dead;
            for (int i = 0; i < 3000; ++i)
                if (rng() % 5 < 3) {
                    dead.push_back(ids[i]);
                    model.erase(ids[i].b);
                }
            R.Remove(dead);
            check(R, model, dead.size(), "random removed");
            const uint64_t rebuilds = R.Stats().rebuilds;
            R.Compact();
            check(R, model, 0, "compacted");
            uint64_t want_slots = 1024;
            while (want_slots < 2 * model.size()) want_slots *= 2;
            EXPECT(R.Stats().capacity == want_slots && R.Stats().rebuilds == rebuilds + 1, "compact: %llu slots",
                   (unsigned long long)R.Stats().capacity);
            std::vector<int64_t> want_stat;
            for (const Digest& d : ids) want_stat.push_back(model.count(d.b) ? model[d.b] : -1);
            EXPECT(R.Stat(ids) == want_stat, "compact: stat of every ID");
            R.Compact(5000);
            EXPECT(R.Stats().capacity == 16384, "compact: min_capacity gives %llu slots",
                   (unsigned long long)R.Stats().capacity);
            check(R, model, 0, "compacted with min_capacity");

            const std::string path = dir + "/repo_persist_test.idx";
            R.Save(path);
            std::unique_ptr<RepoIndex> S = RepoIndex::Restore(e, path);
            check(*S, model, 0, "restored");
            EXPECT(S->Stats().capacity == want_slots && S->Stats().rebuilds == 0, "restore: %llu slots",
                   (unsigned long long)S->Stats().capacity);
            EXPECT(S->Stat(ids) == want_stat, "restore: stat of every ID");
            // the restored index goes on like any other: Put of the removed objects, then a nil-liveset collect
            const Map saved = model;
            std::vector<int64_t> dead_sizes(dead.size(), 7);
            S->Put(dead, dead_sizes);
            for (const Digest& d : dead) model[d.b] = 7;
            check(*S, model, 0, "restored, then put");
            const std::string path2 = dir + "/repo_persist_test2.idx";
            S->Save(path2);
            std::unique_ptr<RepoIndex> T = RepoIndex::Restore(e, path2);
            check(*T, model, 0, "restored again");
            EXPECT(same_set(T->CollectAllList(), model), "restored again: collect all names every object");
            check(*T, Map(), model.size(), "restored again, emptied");
            remove(path.c_str());
            remove(path2.c_str());
            // a missing file: an error, and the engine goes on
            bool threw = false;
            try {
                RepoIndex::Restore(e, path);
            } catch (const Error& err) {
                threw = err.code == RF_EIO;
            }
            EXPECT(threw, "restore of a missing file");
            check(R, saved, 0, "the saved index is untouched");
        }
    } catch (const Error& err) {
        fprintf(stderr, "FAIL: Error %d: %s\n", err.code, err.what());
        return 1;
    }
    if (failures) return 1;
    printf("PASS\n");
    return 0;
}
