// live_mirror_test.cpp -- the GC liveset through the C++ host mirror
// (include/reflow_host.hpp GcLiveset), on the device: TestGC's flow
// (test/evaltest/eval_test.go:353-409) stage by stage -- at the end the
// repository's eight objects lose exactly `unrooted` -- and one random DAG
// with random values and writers, each against Eval.collect (eval.go:791-868)
// worked out here on the host.
#include <cstdio>
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

struct Graph {
    std::vector<uint64_t> ptr{0};
    std::vector<uint32_t> edges;
    std::vector<const Fileset*> value;  // null: no value
    void node(std::initializer_list<uint32_t> e) { node(std::vector<uint32_t>(e)); }
    void node(const std::vector<uint32_t>& e) {
        edges.insert(edges.end(), e.begin(), e.end());
        ptr.push_back(edges.size());
        value.push_back(nullptr);
    }
    size_t n() const { return value.size(); }
};

static void rows_of(const Fileset& v, std::vector<File>& out) {
    if (v.List)
        for (const Fileset& c : *v.List) rows_of(c, out);
    for (const auto& kv : v.Map) out.push_back(kv.second);
}

struct Want {
    std::vector<uint8_t> states;
    uint64_t contributions = 0, nlive_est = 0, nlive = 0, m = 64, k = 1;
    int64_t livebytes = 0;
    std::vector<Digest> ids;  // every row's ID
};

// Eval.collect on the host (eval.go:809-858)
static Want collect(const Graph& g, const std::vector<uint32_t>& roots, const std::vector<uint32_t>& writers) {
    Want w;
    w.states.assign(g.n(), RF_LIVE_UNSEEN);
    std::vector<uint32_t> stack(roots.begin(), roots.end());
    while (!stack.empty()) {
        const uint32_t i = stack.back();
        stack.pop_back();
        if (w.states[i] != RF_LIVE_UNSEEN) continue;
        if (g.value[i]) {
            w.states[i] = RF_LIVE_VALUE;
            continue;
        }
        w.states[i] = RF_LIVE_WALKED;
        for (uint64_t e = g.ptr[i]; e < g.ptr[i + 1]; ++e) stack.push_back(g.edges[e]);
    }
    std::vector<uint32_t> contrib;
    for (uint32_t i = 0; i < g.n(); ++i)
        if (w.states[i] == RF_LIVE_VALUE) contrib.push_back(i);
    contrib.insert(contrib.end(), writers.begin(), writers.end());
    w.contributions = contrib.size();
    for (uint32_t c : contrib) {
        if (!g.value[c]) continue;
        std::vector<File> rows;
        rows_of(*g.value[c], rows);
        w.nlive_est += rows.size();
        std::set<std::pair<std::array<uint8_t, 32>, int64_t>> files;  // Files(): map[File]bool
        for (const File& f : rows) {
            w.ids.push_back(f.ID);
            if (files.insert({f.ID.b, f.Size}).second) {
                ++w.nlive;
                w.livebytes += f.Size;
            }
        }
    }
    if (w.nlive_est) Check(rf_bloom_estimate(w.nlive_est, 0.001, &w.m, &w.k));
    return w;
}

static void compare(GcLiveset& L, const GcLiveset::Result& r, const Want& w, const char* what) {
    EXPECT(L.States() == w.states, "%s: states", what);
    const rf_liveset_stats st = L.Stats();
    EXPECT(st.contributions == w.contributions && st.nlive_est == w.nlive_est && st.nlive == w.nlive &&
               st.livebytes == w.livebytes && st.m == w.m && st.k == w.k,
           "%s: contributions %llu/%llu est %llu/%llu nlive %llu/%llu bytes %lld/%lld m %llu/%llu k %llu/%llu", what,
           (unsigned long long)st.contributions, (unsigned long long)w.contributions,
           (unsigned long long)st.nlive_est, (unsigned long long)w.nlive_est, (unsigned long long)st.nlive,
           (unsigned long long)w.nlive, (long long)st.livebytes, (long long)w.livebytes, (unsigned long long)st.m,
           (unsigned long long)w.m, (unsigned long long)st.k, (unsigned long long)w.k);
    EXPECT(r.nlive == w.nlive && r.livebytes == w.livebytes, "%s: the result's figures", what);
    for (int s = 0; s < 3; ++s) {
        std::vector<uint32_t> want;
        for (uint32_t i = 0; i < w.states.size(); ++i)
            if (w.states[i] == s) want.push_back(i);
        EXPECT(L.List(s) == want && st.counts[s] == want.size(), "%s: list of state %d", what, s);
    }
    for (bool in : r.live.Contains(w.ids)) EXPECT(in, "%s: a live file is not in the filter", what);
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
            // TestGC: 0 pullup, 1 mapPullup, 2 mapCollect, 3 its function's pullup, 4 groupby, 5 its
            // function's collect, 6 the orphan collect, 7 intern, 8 / 9 the functions' arguments
            Graph g;
            g.node({1});
            g.node({2, 3});
            g.node({4, 5});
            g.node({9, 6});
            g.node({7});
            g.node({8});
            g.node({7});
            g.node({});
            g.node({});
            g.node({});
            GcLiveset L(e, g.ptr, g.edges);
            const Fileset interned = files(D, {{"a/x", "x"}, {"a/y", "y"}, {"a/z", "z"}, {"b/1", "1"}, {"b/2", "2"},
                                               {"c/xxx", "xxx"}, {"orphan", "orphan"}, {"unrooted", "unrooted"}});
            Fileset grouped;
            grouped.List = std::vector<Fileset>{files(D, {{"a/x", "x"}, {"a/y", "y"}, {"a/z", "z"}}),
                                                files(D, {{"b/1", "1"}, {"b/2", "2"}}), files(D, {{"c/xxx", "xxx"}})};
            const Fileset result = files(D, {{"x", "x"}, {"y", "y"}, {"z", "z"}, {"1", "1"}, {"2", "2"},
                                             {"xxx", "xxx"}, {"anotherfile", "orphan"}});
            std::vector<Digest> objects;
            std::vector<int64_t> sizes;
            for (const auto& kv : interned.Map) {
                objects.push_back(kv.second.ID);
                sizes.push_back(kv.second.Size);
            }
            auto r0 = L.Collect({0});
            compare(L, r0, collect(g, {0}, {}), "gc nothing done");
            EXPECT(r0.changed && L.Stats().m == 64 && L.Stats().k == 1, "gc nothing done: the empty filter");
            g.value[7] = &interned;
            L.SetValue(7, interned);
            auto r1 = L.Collect({0});
            compare(L, r1, collect(g, {0}, {}), "gc intern done");
            EXPECT(r1.changed && L.Stats().m == 116 && L.Stats().k == 11 && r1.nlive == 8, "gc intern done: (116, 11)");
            EXPECT(r1.live.Collect(objects, sizes).first.empty(), "gc intern done: every object is live");
            g.value[4] = &grouped;
            L.SetValue(4, grouped);
            auto r2 = L.Collect({0});
            compare(L, r2, collect(g, {0}, {}), "gc groupby done");
            EXPECT(r2.changed && r2.nlive == 14, "gc groupby done: nlive %llu", (unsigned long long)r2.nlive);
            g.value[0] = &result;
            L.SetValue(0, result);
            auto r3 = L.Collect({0});
            compare(L, r3, collect(g, {0}, {}), "gc root done");
            EXPECT(r3.changed && L.Stats().m == 101 && L.Stats().k == 11 && r3.nlive == 7, "gc root done: (101, 11)");
            const auto dead = r3.live.Collect(objects, sizes);
            EXPECT(dead.first.size() == 1 && objects[dead.first[0]] == D.FromString("unrooted") && dead.second == 8,
                   "gc root done: %zu objects collected", dead.first.size());
            const std::string js = r3.live.MarshalJSON();
            auto r4 = L.Collect({0});
            EXPECT(!r4.changed && r4.live.MarshalJSON() == js, "gc root done again: unchanged");
            EXPECT(L.Stats().maxlivebytes == 30 && L.Stats().stale_rows == 0, "gc: maxlivebytes %lld",
                   (long long)L.Stats().maxlivebytes);
        }
        {
            // a random DAG (edges point at higher ids), values on a third of the nodes
            std::mt19937 rng(11);
            const uint32_t n = 500;
            Graph g;
            for (uint32_t i = 0; i < n; ++i) {
                std::vector<uint32_t> ed;
                const uint32_t deg = i + 1 < n ? rng() % 5 : 0;
                for (uint32_t d = 0; d < deg; ++d) ed.push_back(i + 1 + rng() % (n - i - 1));
                g.node(ed);
            }
            std::vector<Fileset> vals(n);
            std::vector<uint32_t> nodes;
            std::vector<const Fileset*> ptrs;
            for (uint32_t i = 1; i < n; ++i) {
                if (rng() % 3) continue;
                const uint32_t rows = rng() % 6;
                for (uint32_t r = 0; r < rows; ++r)  // few distinct files: shared between and repeated within values
                    vals[i].Map["p" + std::to_string(r)] = File{D.FromString("f" + std::to_string(rng() % 40)), (int64_t)(rng() % 3)};
                if (rng() % 4 == 0) vals[i].List = std::vector<Fileset>{vals[i], vals[i]};
                g.value[i] = &vals[i];
                nodes.push_back(i);
                ptrs.push_back(&vals[i]);
            }
            GcLiveset L(e, g.ptr, g.edges);
            L.SetValues(nodes, ptrs);
            std::vector<uint32_t> writers;
            for (int w = 0; w < 9; ++w) writers.push_back(rng() % n);
            writers.push_back(writers[0]);
            auto r = L.Collect({0, 3, 3}, writers);
            compare(L, r, collect(g, {0, 3, 3}, writers), "random");
            EXPECT(r.changed, "random: first run");
            EXPECT(!L.Collect({0, 3, 3}, writers).changed, "random: unchanged");
            g.value[nodes[0]] = nullptr;
            L.ClearValues({nodes[0]});
            auto r2 = L.Collect({0, 3, 3}, writers);
            compare(L, r2, collect(g, {0, 3, 3}, writers), "random, a value cleared");
        }
    } catch (const Error& err) {
        fprintf(stderr, "FAIL: Error %d: %s\n", err.code, err.what());
        return 1;
    }
    if (failures) return 1;
    printf("PASS\n");
    return 0;
}
