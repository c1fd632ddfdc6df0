// plan_mirror_test.cpp -- the evaluation plan through the C++ host mirror
// (include/reflow_host.hpp EvalPlan), on the device: a two-branch flow
// merge(extern(exec(val, val)), extern(exec(val, val))) planned from keys on
// the host and from the Eval's graph, then a reject and a NoCacheExtern run,
// each against the states Eval.todo + Eval.lookup give by hand
// (eval.go:902-955, 1163-1269).
#include <cstdio>
#include <string>

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

static std::string show(const std::vector<uint8_t>& st) {
    std::string s;
    for (uint8_t x : st) s += "UTRHD"[x < 5 ? x : 0];
    return s;
}

int main() {
    try {
        Engine e(0);
        Digester D(e);
        FlowArena a;
        // nodes: 0 root, 1 extern0, 2 extern1, 3 exec0, 4 exec1, 5..8 the vals
        std::vector<Flow*> nodes(9);
        for (int b = 0; b < 2; ++b) {
            nodes[5 + 2 * b] = flow::Val(a, one(D.FromString("a" + std::to_string(b))));
            nodes[6 + 2 * b] = flow::Val(a, one(D.FromString("b" + std::to_string(b))));
            nodes[3 + b] = flow::Exec(a, "img", "cmd %s %s # " + std::to_string(b), {nodes[5 + 2 * b], nodes[6 + 2 * b]});
            nodes[3 + b]->Argmap = std::vector<ExecArg>{{false, 0}, {false, 1}, {true, 0}};
            nodes[1 + b] = flow::Extern(a, "s3://out/" + std::to_string(b), nodes[3 + b]);
        }
        nodes[0] = flow::Merge(a, {nodes[1], nodes[2]});
        Eval ev(e);
        ev.Add(nodes[0]);
        ev.Build();
        const std::vector<uint64_t> dep_ptr = {0, 2, 3, 4, 6, 8, 8, 8, 8, 8};
        const std::vector<uint32_t> deps = {1, 2, 3, 4, 5, 6, 7, 8};
        const std::vector<uint8_t> flags = {0,
                                            RF_PLAN_F_CACHEABLE | RF_PLAN_F_EXTERN,
                                            RF_PLAN_F_CACHEABLE | RF_PLAN_F_EXTERN,
                                            RF_PLAN_F_CACHEABLE,
                                            RF_PLAN_F_CACHEABLE,
                                            0, 0, 0, 0};
        std::vector<uint64_t> key_ptr = {0};
        std::vector<Digest> keys;
        std::vector<uint32_t> key_slots;
        for (Flow* f : nodes) {
            const std::vector<Digest> k = ev.CacheKeys(f);
            const std::vector<uint32_t> s = ev.CacheKeySlots(f);
            EXPECT(k.size() == s.size() && !k.empty(), "keys %zu, slots %zu", k.size(), s.size());
            keys.insert(keys.end(), k.begin(), k.end());
            key_slots.insert(key_slots.end(), s.begin(), s.end());
            key_ptr.push_back(keys.size());
        }
        EXPECT(EvalPlan::Check(dep_ptr, deps) == 4, "depth %u", EvalPlan::Check(dep_ptr, deps));
        try {
            EvalPlan::Check({0, 1, 2}, {1, 0});
            EXPECT(false, "a 2-cycle passed the check");
        } catch (const Error& err) {
            EXPECT(err.code == RF_EINVAL, "cycle: code %d", err.code);
        }

        // cached: exec0 under its least concrete key only, extern1 under its first
        Assoc assoc(e, 64);
        const Digest fs_exec0 = D.FromString("fileset of exec0"), fs_ext1 = D.FromString("fileset of extern1");
        const uint64_t last0 = key_ptr[4] - 1;
        assoc.Put(AssocFileset, Digest{}, keys[last0], fs_exec0);
        assoc.Put(AssocFileset, Digest{}, keys[key_ptr[2]], fs_ext1);
        EvalPlan plan(e, dep_ptr, deps, flags, key_ptr, &key_slots);
        EXPECT(plan.Stats().depth == 4 && plan.Stats().n_nodes == 9, "stats at open");
        const std::string want1 = "TRHHUUUUU";  // root waits for extern0; extern0 is ready: exec0 is a hit
        for (int from_graph = 0; from_graph < 2; ++from_graph) {
            if (from_graph)
                plan.Run({0}, ev, nullptr, assoc, AssocFileset);
            else
                plan.Run({0}, keys, nullptr, assoc, AssocFileset);
            EXPECT(show(plan.States()) == want1, "run %d: states %s", from_graph, show(plan.States()).c_str());
            const std::vector<EvalPlan::Hit> hits = plan.Hits();
            EXPECT(hits.size() == 2, "run %d: %zu hits", from_graph, hits.size());
            if (hits.size() == 2) {
                EXPECT(hits[0].node == 2 && hits[0].which == 0 && hits[0].value == fs_ext1 && hits[0].key_found == 1, "extern1's hit");
                const int w = (int)(last0 - key_ptr[3]);
                EXPECT(hits[1].node == 3 && hits[1].which == w && hits[1].value == fs_exec0 && hits[1].key_found == (1u << w), "exec0's hit");
            }
            EXPECT(plan.List(RF_PLAN_TODO) == std::vector<uint32_t>({0}) && plan.List(RF_PLAN_READY) == std::vector<uint32_t>({1}), "lists");
            const rf_eval_plan_stats st = plan.Stats();
            EXPECT(st.counts[RF_PLAN_UNSEEN] == 5 && st.counts[RF_PLAN_HIT] == 2 && st.looked_up == 3 && st.rounds <= st.depth, "stats of run %d", from_graph);
        }
        // extern1's files are missing: it has to run, and so has exec1 beneath it
        plan.Reject({2}, ev, nullptr, assoc, AssocFileset);
        EXPECT(show(plan.States()) == "TRTHTUURR", "after reject: states %s", show(plan.States()).c_str());
        try {
            plan.Reject({1}, keys, nullptr, assoc, AssocFileset);
            EXPECT(false, "rejecting a node that is no hit passed");
        } catch (const Error& err) {
            EXPECT(err.code == RF_EINVAL, "reject of a non-hit: code %d", err.code);
        }
        EXPECT(show(plan.States()) == "TRTHTUURR", "a refused reject changed the states");
        // the same as a fresh run with extern1 invalid
        plan.SetFlags({2}, {RF_PLAN_F_CACHEABLE | RF_PLAN_F_EXTERN | RF_PLAN_F_INVALID});
        plan.Run({0}, keys, nullptr, assoc, AssocFileset);
        EXPECT(show(plan.States()) == "TRTHTUURR", "with extern1 invalid: states %s", show(plan.States()).c_str());
        plan.SetFlags({2}, {RF_PLAN_F_CACHEABLE | RF_PLAN_F_EXTERN});
        // NoCacheExtern: the externs are not looked up; the execs beneath them are clean
        plan.Run({0}, keys, nullptr, assoc, AssocFileset, /*no_cache_extern=*/true);
        EXPECT(show(plan.States()) == "TRTHTUURR", "NoCacheExtern: states %s", show(plan.States()).c_str());
        // exec0 ran: done nodes are left alone and satisfy their consumers
        plan.SetFlags({3}, {RF_PLAN_F_CACHEABLE | RF_PLAN_F_DONE});
        Liveset live(e, 4096, 5);  // empty: every key is filtered, nothing hits
        plan.Run({0, 0}, keys, &live, assoc, AssocFileset);
        EXPECT(show(plan.States()) == "TRTDTUURR", "done exec0, empty liveset: states %s", show(plan.States()).c_str());
        EXPECT(plan.Stats().keys_probed == 0 && plan.Stats().keys_filtered > 0, "liveset figures");
    } catch (const Error& err) {
        fprintf(stderr, "error %d: %s\n", err.code, err.what());
        return 2;
    }
    if (failures) return 1;
    printf("PASS\n");
    return 0;
}
