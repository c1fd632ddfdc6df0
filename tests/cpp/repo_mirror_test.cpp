// repo_mirror_test.cpp -- the repository index through the C++ host mirror
// (include/reflow_host.hpp RepoIndex), on the device: TestCacheLookupMissing's
// shape (test/evaltest/eval_test.go:279-312: the value's x, y, z of size 1, x
// deleted: one missing file, one byte), Put's first-wins rule, TestGC's
// objects collected with the GcLiveset's filter, and random values and deps
// against missing() / NeedTransfer worked out here on the host.
#include <cstdio>
#include <map>
#include <random>
#include <set>
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

static void rows_of(const Fileset& v, std::vector<File>& out) {
    if (v.List)
        for (const Fileset& c : *v.List) rows_of(c, out);
    for (const auto& kv : v.Map) out.push_back(kv.second);
}

using Key = std::pair<std::array<uint8_t, 32>, int64_t>;

// missing() over groups of rows against a plain map: Files() per group, first occurrence order
static RepoIndex::Report model(const std::map<std::array<uint8_t, 32>, int64_t>& repo,
                               const std::vector<std::vector<File>>& groups) {
    RepoIndex::Report w;
    uint64_t row = 0;
    w.miss_ptr.push_back(0);
    for (const auto& g : groups) {
        std::set<Key> seen;
        uint32_t files = 0, missing = 0;
        int64_t bytes = 0;
        for (const File& f : g) {
            if (seen.insert({f.ID.b, f.Size}).second) {
                ++files;
                if (!repo.count(f.ID.b)) {
                    ++missing;
                    bytes += f.Size;
                    w.miss_rows.push_back(row);
                    w.files.push_back(f);
                }
            }
            ++row;
        }
        w.n_files.push_back(files);
        w.n_missing.push_back(missing);
        w.missing_bytes.push_back(bytes);
        w.miss_ptr.push_back(w.files.size());
    }
    return w;
}

static bool same_files(const std::vector<File>& a, const std::vector<File>& b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); ++i)
        if (!(a[i].ID == b[i].ID) || a[i].Size != b[i].Size) return false;
    return true;
}

static void compare(const RepoIndex::Report& got, const RepoIndex::Report& want, bool rows, const char* what) {
    EXPECT(got.n_files == want.n_files, "%s: n_files", what);
    EXPECT(got.n_missing == want.n_missing, "%s: n_missing", what);
    EXPECT(got.missing_bytes == want.missing_bytes, "%s: missing_bytes", what);
    EXPECT(got.miss_ptr == want.miss_ptr, "%s: miss_ptr", what);
    EXPECT(same_files(got.files, want.files), "%s: the list (%zu / %zu files)", what, got.files.size(),
           want.files.size());
    if (rows) EXPECT(got.miss_rows == want.miss_rows, "%s: miss_rows", what);
}

static Fileset files(Digester& D, std::initializer_list<std::pair<const char*, const char*>> specs) {
    Fileset v;
    for (const auto& s : specs) v.Map[s.first] = File{D.FromString(s.second), (int64_t)std::string(s.second).size()};
    return v;
}

int main() {
    try {
        Engine e(0);
        Digester D(e);
        {
            // TestCacheLookupMissing: the cached value's files x, y, z; the repository lost x
            RepoIndex R(e);
            const Fileset value = files(D, {{"x", "x"}, {"y", "y"}, {"z", "z"}});
            std::vector<File> rows;
            rows_of(value, rows);
            std::vector<Digest> ids;
            std::vector<int64_t> sizes;
            for (const File& f : rows) {
                ids.push_back(f.ID);
                sizes.push_back(f.Size);
            }
            EXPECT(R.Put(ids, sizes) == std::vector<int>(3, RF_OK), "put");
            EXPECT(R.Missing(std::vector<Fileset>{value}).n_missing == std::vector<uint32_t>{0}, "all present");
            EXPECT(R.Remove({D.FromString("x")}) == std::vector<bool>{true}, "remove x");
            const RepoIndex::Report rep = R.Missing(std::vector<Fileset>{value});
            EXPECT(rep.n_files == std::vector<uint32_t>{3} && rep.n_missing == std::vector<uint32_t>{1} &&
                       rep.missing_bytes == std::vector<int64_t>{1} && rep.files.size() == 1 &&
                       rep.files[0].ID == D.FromString("x") && rep.files[0].Size == 1,
                   "lookup missing: %u files, %u missing", rep.n_files[0], rep.n_missing[0]);
            EXPECT(R.Stat({D.FromString("x"), D.FromString("y")}) == (std::vector<int64_t>{-1, 1}), "stat");
            // first wins: y again with another size, a new ID twice with two sizes, x again (a fresh object)
            const std::vector<int> st = R.Put({D.FromString("y"), D.FromString("w"), D.FromString("w"), D.FromString("x")},
                                              {2, 5, 6, 9});
            EXPECT(st == (std::vector<int>{RF_EINTEGRITY, RF_OK, RF_EINTEGRITY, RF_OK}), "put: first wins");
            EXPECT(R.Stat({D.FromString("y"), D.FromString("w"), D.FromString("x")}) == (std::vector<int64_t>{1, 5, 9}),
                   "put: the stored sizes");
            const rf_repo_stats s = R.Stats();
            EXPECT(s.objects == 4 && s.bytes == 1 + 1 + 5 + 9 && s.tombstones == 0, "stats: %llu objects",
                   (unsigned long long)s.objects);
            const auto all = R.CollectAll();
            EXPECT(all.first == 4 && all.second == 16 && R.Stats().objects == 0, "collect all");
        }
        {
            // TestGC's repository: after the root is done Collect removes exactly `unrooted`
            const std::vector<uint64_t> ptr{0, 1, 1};
            const std::vector<uint32_t> edges{1};
            GcLiveset L(e, ptr, edges);
            const Fileset interned = files(D, {{"a/x", "x"}, {"a/y", "y"}, {"a/z", "z"}, {"b/1", "1"}, {"b/2", "2"},
                                               {"c/xxx", "xxx"}, {"orphan", "orphan"}, {"unrooted", "unrooted"}});
            const Fileset result = files(D, {{"x", "x"}, {"y", "y"}, {"z", "z"}, {"1", "1"}, {"2", "2"},
                                             {"xxx", "xxx"}, {"anotherfile", "orphan"}});
            RepoIndex R(e);
            std::vector<Digest> ids;
            std::vector<int64_t> sizes;
            for (const auto& kv : interned.Map) {
                ids.push_back(kv.second.ID);
                sizes.push_back(kv.second.Size);
            }
            R.Put(ids, sizes);
            L.SetValue(1, interned);
            // node 0 (an exec) is ready: its dep's value is all in the repository
            RepoIndex::Report nt = R.NeedTransfer(L, {0, 1});
            EXPECT(nt.status == (std::vector<int>{RF_OK, RF_OK}) && nt.n_files == (std::vector<uint32_t>{8, 0}) &&
                       nt.n_missing == (std::vector<uint32_t>{0, 0}),
                   "need transfer: nothing to move");
            L.SetValue(0, result);
            L.Collect({0});
            const auto gone = R.Collect(L);
            EXPECT(gone.first == 1 && gone.second == 8, "collect: %llu objects", (unsigned long long)gone.first);
            EXPECT(R.Stat({D.FromString("unrooted"), D.FromString("orphan")}) == (std::vector<int64_t>{-1, 6}),
                   "collect: unrooted is gone");
            nt = R.NeedTransfer(L, {0});
            EXPECT(nt.n_files == std::vector<uint32_t>{8} && nt.n_missing == std::vector<uint32_t>{1} &&
                       nt.missing_bytes == std::vector<int64_t>{8} && nt.files.size() == 1 &&
                       nt.files[0].ID == D.FromString("unrooted"),
                   "need transfer: unrooted has to move");
        }
        {
            // random values over few distinct files; deps with and without values
            std::mt19937 rng(23);
            const uint32_t n = 300;
            std::vector<uint64_t> ptr{0};
            std::vector<uint32_t> edges;
            for (uint32_t i = 0; i < n; ++i) {
                const uint32_t deg = i + 1 < n ? rng() % 4 : 0;
                for (uint32_t d = 0; d < deg; ++d) edges.push_back(i + 1 + rng() % (n - i - 1));
                if (deg && rng() % 5 == 0) edges.push_back(edges.back());  // a dep listed twice
                ptr.push_back(edges.size());
            }
            std::vector<Fileset> vals(n);
            std::vector<bool> has(n, false);
            std::vector<uint32_t> nodes;
            std::vector<const Fileset*> ptrs;
            for (uint32_t i = 0; i < n; ++i) {
                if (rng() % 4 == 0) continue;
                const uint32_t rows = rng() % 6;
                for (uint32_t r = 0; r < rows; ++r)
                    vals[i].Map["p" + std::to_string(r)] =
                        File{D.FromString("f" + std::to_string(rng() % 60)), (int64_t)(rng() % 3)};
                if (rng() % 4 == 0) vals[i].List = std::vector<Fileset>{vals[i], vals[i]};
                has[i] = true;
                nodes.push_back(i);
                ptrs.push_back(&vals[i]);
            }
            GcLiveset L(e, ptr, edges);
            L.SetValues(nodes, ptrs);
            RepoIndex R(e);
            std::map<std::array<uint8_t, 32>, int64_t> repo;
            std::vector<Digest> ids;
            std::vector<int64_t> sizes;
            for (int f = 0; f < 60; f += 2) {  // the even files, each with one size
                ids.push_back(D.FromString("f" + std::to_string(f)));
                sizes.push_back(f % 3);
                repo[ids.back().b] = sizes.back();
            }
            R.Put(ids, sizes);
            std::vector<std::vector<File>> groups;
            for (const Fileset* v : ptrs) {
                groups.emplace_back();
                rows_of(*v, groups.back());
            }
            compare(R.Missing(ptrs), model(repo, groups), true, "random missing");
            // NeedTransfer over every node: a dep without a value fails its group alone
            std::vector<uint32_t> every;
            std::vector<std::vector<File>> deps;
            std::vector<int> status;
            for (uint32_t i = 0; i < n; ++i) {
                every.push_back(i);
                deps.emplace_back();
                bool ok = true;
                for (uint64_t x = ptr[i]; x < ptr[i + 1]; ++x) ok = ok && has[edges[x]];
                status.push_back(ok ? RF_OK : RF_EPRECONDITION);
                if (!ok) continue;
                for (uint64_t x = ptr[i]; x < ptr[i + 1]; ++x) rows_of(vals[edges[x]], deps.back());
            }
            const RepoIndex::Report nt = R.NeedTransfer(L, every);
            compare(nt, model(repo, deps), false, "random need transfer");
            EXPECT(nt.status == status, "random need transfer: status");
        }
    } catch (const Error& err) {
        fprintf(stderr, "FAIL: Error %d: %s\n", err.code, err.what());
        return 1;
    }
    if (failures) return 1;
    printf("PASS\n");
    return 0;
}
