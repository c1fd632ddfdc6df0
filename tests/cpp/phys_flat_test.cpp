// phys_flat_test.cpp -- the physical keys on the host: rf_physkeys_flat
// (reflow_amd/csrc/physkeys_flat.cpp), which runs the tiled code the kernels of
// k13_physkeys.hip run (phys_emit.h: node lengths / scan / per-entry emit,
// segment table / tiled gather), against a naive sequential form written here:
// a recursive Fileset material, a plain concatenation per consumer and its own
// scalar SHA-256.  Values go in as a tree and as forest arrays built here in
// closing order.  No library, no device; built plain and under
// AddressSanitizer + UBSan (reflow_amd/csrc/Makefile phys_flat_test, run by
// tests/test_physkeys_flat.py).
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <random>
#include <string>
#include <vector>

#include "reflow_hip.h"

static int g_fail = 0;
#define CHECK(c)                                                \
    do {                                                        \
        if (!(c)) {                                             \
            printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
            ++g_fail;                                           \
        }                                                       \
    } while (0)

// ---- a SHA-256 of its own (FIPS 180-4) ----------------------------------------
static const uint32_t K[64] = {
    0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01,
    0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc,
    0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147,
    0x06ca6351, 0x14292967, 0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85,
    0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08,
    0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208,
    0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};
static uint32_t ror(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }
static std::string sha256(const std::string& m) {
    uint32_t h[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
    std::string p = m;
    p.push_back((char)0x80);
    while (p.size() % 64 != 56) p.push_back(0);
    for (int i = 7; i >= 0; --i) p.push_back((char)(((uint64_t)m.size() * 8) >> (8 * i)));
    for (size_t b = 0; b < p.size(); b += 64) {
        uint32_t w[64];
        for (int t = 0; t < 16; ++t)
            w[t] = (uint32_t)(uint8_t)p[b + 4 * t] << 24 | (uint32_t)(uint8_t)p[b + 4 * t + 1] << 16 |
                   (uint32_t)(uint8_t)p[b + 4 * t + 2] << 8 | (uint8_t)p[b + 4 * t + 3];
        for (int t = 16; t < 64; ++t)
            w[t] = w[t - 16] + (ror(w[t - 15], 7) ^ ror(w[t - 15], 18) ^ (w[t - 15] >> 3)) + w[t - 7] +
                   (ror(w[t - 2], 17) ^ ror(w[t - 2], 19) ^ (w[t - 2] >> 10));
        uint32_t a = h[0], bb = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
        for (int t = 0; t < 64; ++t) {
            const uint32_t t1 = hh + (ror(e, 6) ^ ror(e, 11) ^ ror(e, 25)) + ((e & f) ^ (~e & g)) + K[t] + w[t];
            const uint32_t t2 = (ror(a, 2) ^ ror(a, 13) ^ ror(a, 22)) + ((a & bb) ^ (a & c) ^ (bb & c));
            hh = g, g = f, f = e, e = d + t1, d = c, c = bb, bb = a, a = t1 + t2;
        }
        h[0] += a, h[1] += bb, h[2] += c, h[3] += d, h[4] += e, h[5] += f, h[6] += g, h[7] += hh;
    }
    std::string out;
    for (int i = 0; i < 8; ++i)
        for (int b = 3; b >= 0; --b) out.push_back((char)(h[i] >> (8 * b)));
    return out;
}

// ---- values ---------------------------------------------------------------------
struct Val {
    std::vector<std::pair<std::string, std::string>> map;  // (path, id32), in any order, paths distinct
    std::vector<Val> list;
};

static std::string naive_material(const Val& v) {
    std::string out;
    if (!v.list.empty()) {  // List wins
        for (const Val& c : v.list) out += naive_material(c);
        return out;
    }
    auto m = v.map;
    std::sort(m.begin(), m.end());
    for (const auto& e : m) out += e.first + std::string("\x00\x05", 2) + e.second;
    return out;
}

static Val random_val(std::mt19937_64& rng, int depth, uint32_t max_entries, uint32_t max_path) {
    Val v;
    if (rng() % 5 != 0) {
        const uint32_t n = (uint32_t)(rng() % (max_entries + 1));
        for (uint32_t i = 0; i < n; ++i) {
            std::string p;
            const uint32_t len = (uint32_t)(rng() % (max_path + 1));
            for (uint32_t k = 0; k < len; ++k) p.push_back((char)(rng() % 256));
            p += "#" + std::to_string(i);  // distinct
            std::string id;
            for (int k = 0; k < 32; ++k) id.push_back((char)(rng() % 256));
            v.map.emplace_back(p, id);
        }
    }
    if (depth < 3 && rng() % 5 < 2) {
        const uint32_t n = 1 + (uint32_t)(rng() % 3);
        for (uint32_t i = 0; i < n; ++i) v.list.push_back(random_val(rng, depth + 1, max_entries, max_path));
    }
    return v;
}

// rf_fileset_tree over the values, nodes in pre-order, Maps in the order given
struct Tree {
    std::vector<uint64_t> list_ptr, entry_ptr{0};
    std::vector<uint32_t> list_child, path_lens;
    std::vector<std::vector<char>> store;
    std::vector<const char*> paths;
    std::vector<uint8_t> ids;
    std::vector<int64_t> sizes;
    std::vector<std::vector<uint32_t>> kids;
    uint32_t add(const Val& v) {
        const uint32_t node = (uint32_t)kids.size();
        kids.emplace_back();
        for (const auto& e : v.map) {
            store.emplace_back(e.first.begin(), e.first.end());
            if (store.back().empty()) store.back().push_back(0);
            path_lens.push_back((uint32_t)e.first.size());
            ids.insert(ids.end(), e.second.begin(), e.second.end());
            sizes.push_back(1);
        }
        entry_ptr.push_back(path_lens.size());
        for (const Val& c : v.list) {
            const uint32_t k = add(c);
            kids[node].push_back(k);
        }
        return node;
    }
    rf_fileset_tree c() {
        list_ptr.assign(1, 0);
        list_child.clear();
        for (const auto& k : kids) {
            list_child.insert(list_child.end(), k.begin(), k.end());
            list_ptr.push_back(list_child.size());
        }
        paths.clear();
        for (const auto& s : store) paths.push_back(s.data());
        rf_fileset_tree t{};
        t.n_nodes = kids.size();
        t.list_ptr = list_ptr.data();
        t.list_child = list_child.data();
        t.entry_ptr = entry_ptr.data();
        t.paths = paths.data();
        t.path_lens = path_lens.data();
        t.ids32 = ids.data();
        t.sizes = sizes.data();
        return t;
    }
};

// the arrays of rf_fileset_forest_copy: closing order, Maps bytewise ordered
struct Forest {
    std::vector<uint64_t> doc_node_ptr{0}, entry_ptr{0}, path_off{0};
    std::vector<uint32_t> node_depth;
    std::vector<uint8_t> paths, ids;
    void node(const Val& v, uint32_t depth) {
        for (const Val& c : v.list) node(c, depth + 1);
        auto m = v.map;
        std::sort(m.begin(), m.end());
        for (const auto& e : m) {
            paths.insert(paths.end(), e.first.begin(), e.first.end());
            path_off.push_back(paths.size());
            ids.insert(ids.end(), e.second.begin(), e.second.end());
        }
        node_depth.push_back(depth);
        entry_ptr.push_back(path_off.size() - 1);
    }
    void doc(const Val& v) {
        node(v, 0);
        doc_node_ptr.push_back(node_depth.size());
    }
    rf_forest_arrays c() const {
        rf_forest_arrays a{};
        a.n_docs = doc_node_ptr.size() - 1;
        a.doc_node_ptr = doc_node_ptr.data();
        a.node_depth = node_depth.data();
        a.entry_ptr = entry_ptr.data();
        a.path_off = path_off.data();
        a.paths = paths.data();
        a.ids32 = ids.data();
        return a;
    }
};

struct Graph {
    std::vector<uint64_t> dep_ptr{0}, phys_row, suffix_ptr{0};
    std::vector<uint32_t> deps;
    std::string suffix;
    uint64_t n() const { return phys_row.size(); }
};

static void run_case(uint64_t seed, uint32_t n, uint32_t max_entries, uint32_t max_path, uint32_t max_suffix) {
    std::mt19937_64 rng(seed);
    Graph g;
    uint64_t n_rows = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t k = i ? (uint32_t)(rng() % 4) : 0;
        for (uint32_t j = 0; j < k; ++j) g.deps.push_back((uint32_t)(rng() % i));
        if (k && rng() % 4 == 0) g.deps.push_back(g.deps.back());  // a dep twice
        g.dep_ptr.push_back(g.deps.size());
        g.phys_row.push_back(rng() % 3 ? n_rows++ : RF_PHYS_NO_ROW);
        const uint32_t sl = (uint32_t)(rng() % (max_suffix + 1));
        for (uint32_t j = 0; j < sl; ++j) g.suffix.push_back((char)(rng() % 256));
        g.suffix_ptr.push_back(g.suffix.size());
    }
    n_rows += 2;
    // values: most nodes once, some twice (the last counts), some documents skipped
    std::vector<uint32_t> nodes;
    std::vector<Val> vals;
    for (uint32_t i = 0; i < n; ++i)
        for (int rep = 0; rep < 2; ++rep)
            if (rng() % 10 < (rep ? 1u : 7u)) {
                nodes.push_back(rng() % 12 ? i : 0xffffffffu);
                vals.push_back(random_val(rng, 0, max_entries, max_path));
            }
    std::shuffle(nodes.begin(), nodes.end(), rng);
    // naive: the last document of a node is its value
    std::vector<int64_t> val_of(n, -1);
    std::vector<std::string> mat(vals.size());
    for (size_t d = 0; d < vals.size(); ++d) {
        mat[d] = nodes[d] == 0xffffffffu ? std::string() : naive_material(vals[d]);
        if (nodes[d] != 0xffffffffu) val_of[nodes[d]] = (int64_t)d;
    }
    std::vector<uint8_t> want(32 * n_rows, 0xa5);
    for (uint32_t i = 0; i < n; ++i) {
        if (g.phys_row[i] == RF_PHYS_NO_ROW) continue;
        std::string m;
        bool ok = true;
        for (uint64_t e = g.dep_ptr[i]; e < g.dep_ptr[i + 1]; ++e) {
            if (val_of[g.deps[e]] < 0)
                ok = false;
            else
                m += mat[(size_t)val_of[g.deps[e]]];
        }
        m += g.suffix.substr(g.suffix_ptr[i], g.suffix_ptr[i + 1] - g.suffix_ptr[i]);
        const std::string d = ok ? sha256(m) : std::string(32, 0);
        memcpy(want.data() + 32 * g.phys_row[i], d.data(), 32);
    }
    Tree tree;
    std::vector<uint32_t> roots;
    Forest forest;
    for (const Val& v : vals) {
        roots.push_back(tree.add(v));
        forest.doc(v);
    }
    const rf_fileset_tree t = tree.c();
    const rf_forest_arrays fa = forest.c();
    for (int form = 0; form < 2; ++form) {
        std::vector<uint8_t> keys(32 * n_rows, 0xa5);
        std::vector<uint64_t> offs(vals.size() + 1, 0);
        uint64_t need = 0;
        auto call = [&](uint8_t* out, uint64_t cap) {
            return rf_physkeys_flat(g.n(), g.dep_ptr.data(), g.deps.data(), g.phys_row.data(), g.suffix_ptr.data(),
                                    reinterpret_cast<const uint8_t*>(g.suffix.data()), nodes.data(), nodes.size(),
                                    form ? &fa : nullptr, form ? nullptr : &t, form ? nullptr : roots.data(), keys.data(),
                                    n_rows, out, cap, offs.data(), &need);
        };
        int rc = call(nullptr, 0);
        CHECK(rc == RF_OK || need > 0);
        std::vector<uint8_t> out(need ? need : 1);
        rc = call(out.data(), need);
        CHECK(rc == RF_OK);
        if (rc != RF_OK) {
            printf("  seed %llu form %d: %s\n", (unsigned long long)seed, form, rf_last_error());
            continue;
        }
        CHECK(keys == want);
        for (size_t d = 0; d < vals.size(); ++d) {
            const std::string got(reinterpret_cast<const char*>(out.data()) + offs[d], offs[d + 1] - offs[d]);
            CHECK(got == mat[d]);
        }
    }
}

int main() {
    // known answer of the test's own SHA-256
    const std::string e = sha256("");
    CHECK((uint8_t)e[0] == 0xe3 && (uint8_t)e[1] == 0xb0 && (uint8_t)e[31] == 0x55);
    for (uint64_t seed = 1; seed <= 40; ++seed) run_case(seed, 1 + seed % 60, 6, 12, 20);
    // materials that cross gather tiles: long paths, many entries, long suffixes
    for (uint64_t seed = 100; seed < 106; ++seed) run_case(seed, 24, 40, 700, 9000);
    run_case(200, 6, 2, 13000, 0);
    // refusals leave the outputs alone
    {
        const uint64_t dep_ptr[3] = {0, 0, 1}, rows[2] = {0, 0}, sp[3] = {0, 0, 0}, bad_sp[3] = {0, 2, 1};
        const uint64_t ok_rows[2] = {RF_PHYS_NO_ROW, 5};
        const uint32_t deps[1] = {0};
        uint8_t keys[64];
        memset(keys, 0x5a, sizeof keys);
        uint64_t need = 7;
        CHECK(rf_physkeys_flat(2, dep_ptr, deps, rows, sp, nullptr, nullptr, 0, nullptr, nullptr, nullptr, keys, 2, nullptr,
                               0, nullptr, &need) == RF_EINVAL);  // a row twice
        CHECK(rf_physkeys_flat(2, dep_ptr, deps, ok_rows, bad_sp, nullptr, nullptr, 0, nullptr, nullptr, nullptr, keys, 2,
                               nullptr, 0, nullptr, &need) == RF_EINVAL);  // suffix pointers
        CHECK(rf_physkeys_flat(2, dep_ptr, deps, ok_rows, sp, nullptr, nullptr, 0, nullptr, nullptr, nullptr, keys, 2,
                               nullptr, 0, nullptr, &need) == RF_EINVAL);  // row 5 of 2
        const uint32_t self[1] = {1};
        CHECK(rf_physkeys_flat(2, dep_ptr, self, ok_rows, sp, nullptr, nullptr, 0, nullptr, nullptr, nullptr, keys, 8,
                               nullptr, 0, nullptr, &need) == RF_EINVAL);  // a cycle
        for (uint8_t b : keys) CHECK(b == 0x5a);
    }
    if (g_fail) {
        printf("%d checks failed\n", g_fail);
        return 1;
    }
    printf("PASS\n");
    return 0;
}
