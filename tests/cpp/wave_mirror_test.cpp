// wave_mirror_test.cpp -- the evaluation waves through the C++ host mirror
// (include/reflow_host.hpp EvalWave), on the device: the two-branch flow
// merge(extern(exec(val, val)), extern(exec(val, val))) evaluated bottom-up
// from keys on the host and from the Eval's graph, with a reject, refusals,
// NoCacheExtern and a liveset, and continued top-down from an EvalPlan -- each
// against the states Eval.todo + Eval.lookup give by hand
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

using Ids = std::vector<uint32_t>;

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
        {  // the consumer CSR, on the host alone
            const auto cons = EvalWave::Consumers(dep_ptr, deps);
            EXPECT(cons.first == std::vector<uint64_t>({0, 0, 1, 2, 3, 4, 5, 6, 7, 8}), "cons_ptr");
            EXPECT(cons.second == Ids({0, 0, 1, 2, 3, 3, 4, 4}), "cons");
            try {
                EvalWave::Consumers({0, 1, 2}, {1, 0});
                EXPECT(false, "a 2-cycle passed");
            } catch (const Error& err) {
                EXPECT(err.code == RF_EINVAL, "cycle: code %d", err.code);
            }
        }

        // cached: exec0 under its least concrete key only, extern1 under its first
        Assoc assoc(e, 64);
        const Digest fs_exec0 = D.FromString("fileset of exec0"), fs_ext1 = D.FromString("fileset of extern1");
        const uint64_t last0 = key_ptr[4] - 1;
        const int w0 = (int)(last0 - key_ptr[3]);
        assoc.Put(AssocFileset, Digest{}, keys[last0], fs_exec0);
        assoc.Put(AssocFileset, Digest{}, keys[key_ptr[2]], fs_ext1);
        EvalWave wave(e, dep_ptr, deps, flags, key_ptr, &key_slots);
        EXPECT(wave.Stats().depth == 4 && wave.Stats().n_nodes == 9 && wave.Stats().n_deps == 8 && wave.Stats().mode == 0,
               "stats at open");
        try {
            wave.Step({5}, keys, nullptr, assoc, AssocFileset);
            EXPECT(false, "a step before any begin passed");
        } catch (const Error& err) {
            EXPECT(err.code == RF_EPRECONDITION, "step before begin: code %d", err.code);
        }
        for (int from_graph = 0; from_graph < 2; ++from_graph) {
            // wave 0: the vals, which nothing waits on; no lookups on the way down
            if (from_graph)
                wave.Begin({0, 0}, ev, nullptr, assoc, AssocFileset);
            else
                wave.Begin({0}, keys, nullptr, assoc, AssocFileset);
            EXPECT(show(wave.States()) == "TTTTTRRRR", "begin %d: states %s", from_graph, show(wave.States()).c_str());
            rf_eval_wave_stats st = wave.Stats();
            EXPECT(st.mode == 1 && st.waves == 1 && st.last_wave == 4 && st.looked_up == 0 && st.rounds <= st.depth,
                   "stats of begin %d", from_graph);
            EXPECT(wave.List(RF_PLAN_READY, RF_WAVE_LAST) == Ids({5, 6, 7, 8}), "wave 0");
            // the vals are done: the execs are looked up -- exec0 hits under its last key, exec1 misses
            if (from_graph)
                wave.Step({5, 6, 7, 8}, ev, nullptr, assoc, AssocFileset);
            else
                wave.Step({8, 7, 6, 5, 5}, keys, nullptr, assoc, AssocFileset);
            EXPECT(show(wave.States()) == "TTTHRDDDD", "step 1/%d: states %s", from_graph, show(wave.States()).c_str());
            std::vector<EvalWave::Hit> hits = wave.Hits(RF_WAVE_LAST);
            EXPECT(hits.size() == 1, "step 1: %zu hits", hits.size());
            if (hits.size() == 1)
                EXPECT(hits[0].node == 3 && hits[0].which == w0 && hits[0].value == fs_exec0 &&
                           hits[0].key_found == (1u << w0), "exec0's hit");
            st = wave.Stats();
            EXPECT(st.waves == 2 && st.last_wave == 2 && st.looked_up == 2 && st.counts[RF_PLAN_DONE] == 4, "stats of step 1");
            // a step naming a node that still waits is refused and changes nothing
            try {
                wave.Step({3, 1}, keys, nullptr, assoc, AssocFileset);
                EXPECT(false, "a step naming a TODO node passed");
            } catch (const Error& err) {
                EXPECT(err.code == RF_EINVAL, "step of a TODO node: code %d", err.code);
            }
            EXPECT(show(wave.States()) == "TTTHRDDDD" && wave.Stats().waves == 2, "a refused step changed the object");
            // exec0's hit is accepted, exec1 ran: the externs -- extern1 is cached, extern0 is not
            wave.Step({3, 4}, keys, nullptr, assoc, AssocFileset);
            EXPECT(show(wave.States()) == "TRHDDDDDD", "step 2/%d: states %s", from_graph, show(wave.States()).c_str());
            hits = wave.Hits();
            EXPECT(hits.size() == 1 && hits[0].node == 2 && hits[0].which == 0 && hits[0].value == fs_ext1 &&
                       hits[0].key_found == 1, "extern1's hit");
            // extern1's files are missing: it has to run
            wave.Reject({2});
            EXPECT(show(wave.States()) == "TRRDDDDDD", "after reject: states %s", show(wave.States()).c_str());
            EXPECT(wave.List(RF_PLAN_READY, RF_WAVE_LAST) == Ids({1, 2}), "a rejected hit stays a member of its wave");
            try {
                wave.Reject({1});
                EXPECT(false, "rejecting a node that is no hit passed");
            } catch (const Error& err) {
                EXPECT(err.code == RF_EINVAL, "reject of a non-hit: code %d", err.code);
            }
            EXPECT(show(wave.States()) == "TRRDDDDDD", "a refused reject changed the states");
            wave.Step({}, keys, nullptr, assoc, AssocFileset);  // nothing finished: an empty wave
            EXPECT(show(wave.States()) == "TRRDDDDDD" && wave.Stats().last_wave == 0 && wave.Stats().waves == 4, "empty step");
            wave.Step({1, 2, 2}, keys, nullptr, assoc, AssocFileset);
            EXPECT(show(wave.States()) == "RDDDDDDDD" && wave.List(RF_PLAN_READY, RF_WAVE_LAST) == Ids({0}), "the root's wave");
            wave.Step({0}, keys, nullptr, assoc, AssocFileset);
            EXPECT(show(wave.States()) == "DDDDDDDDD" && wave.Stats().last_wave == 0 && wave.Stats().waves == 6, "the end");
        }
        // NoCacheExtern: the externs are not looked up (eval.go:1173); the execs are
        wave.Begin({0}, keys, nullptr, assoc, AssocFileset, /*no_cache_extern=*/true);
        wave.Step({5, 6, 7, 8}, keys, nullptr, assoc, AssocFileset);
        EXPECT(show(wave.States()) == "TTTHRDDDD", "NoCacheExtern, execs: states %s", show(wave.States()).c_str());
        wave.Step({3, 4}, keys, nullptr, assoc, AssocFileset);
        EXPECT(show(wave.States()) == "TRRDDDDDD" && wave.Stats().looked_up == 0, "NoCacheExtern, externs: states %s",
               show(wave.States()).c_str());
        // exec0 ran before: flagged done it is left alone and satisfies extern0 from the start
        wave.SetFlags({3}, {RF_PLAN_F_CACHEABLE | RF_PLAN_F_DONE});
        Liveset live(e, 4096, 5);  // empty: every key is filtered, nothing hits
        wave.Begin({0}, keys, &live, assoc, AssocFileset);
        EXPECT(show(wave.States()) == "TRTDTUURR", "done exec0, empty liveset: states %s", show(wave.States()).c_str());
        EXPECT(wave.Stats().keys_probed == 0 && wave.Stats().keys_filtered > 0 && wave.Stats().looked_up == 1, "liveset figures");
        wave.SetFlags({3}, {RF_PLAN_F_CACHEABLE});

        // the top-down hand-over: the plan's READY list is wave 0, and nothing is looked up after it
        EvalPlan plan(e, dep_ptr, deps, flags, key_ptr, &key_slots);
        plan.Run({0}, keys, nullptr, assoc, AssocFileset);
        EXPECT(show(plan.States()) == "TRHHUUUUU", "plan: states %s", show(plan.States()).c_str());
        for (int on_device = 0; on_device < 2; ++on_device) {
            if (on_device)
                wave.BeginStates(plan);
            else
                wave.BeginStates(plan.States());
            EXPECT(show(wave.States()) == "TRDDUUUUU", "hand-over %d: states %s", on_device, show(wave.States()).c_str());
            EXPECT(wave.List(RF_PLAN_READY, RF_WAVE_LAST) == plan.List(RF_PLAN_READY) && wave.Stats().mode == 2, "wave 0 of the hand-over");
            wave.Step({1});
            EXPECT(show(wave.States()) == "RDDDUUUUU" && wave.Stats().looked_up == 0, "hand-over, step 1: states %s",
                   show(wave.States()).c_str());
            wave.Step({0});
            EXPECT(show(wave.States()) == "DDDDUUUUU" && wave.Stats().last_wave == 0, "hand-over, the end");
        }
        wave.BeginStates(std::vector<uint8_t>({1, 4, 4, 0, 4, 4, 4, 4, 4}));  // an UNSEEN node under a DONE one: fine
        EXPECT(show(wave.States()) == "RDDUDDDDD", "states given by hand: %s", show(wave.States()).c_str());
        for (uint8_t bad : {(uint8_t)RF_PLAN_READY, (uint8_t)5}) {  // extern0 READY over an UNSEEN exec0; no such state
            try {
                wave.BeginStates(std::vector<uint8_t>({1, bad, 4, 0, 4, 4, 4, 4, 4}));
                EXPECT(false, "begin_states with byte %d passed", bad);
            } catch (const Error& err) {
                EXPECT(err.code == RF_EINVAL, "begin_states: code %d", err.code);
            }
            EXPECT(show(wave.States()) == "RDDUDDDDD" && wave.Stats().last_wave == 1, "states after the refusal: %s",
                   show(wave.States()).c_str());
        }
    } catch (const Error& err) {
        fprintf(stderr, "error %d: %s\n", err.code, err.what());
        return 2;
    }
    if (failures) return 1;
    printf("PASS\n");
    return 0;
}
