// json_parse_test.cpp -- the Fileset unmarshal on the host: json_parse.h's
// sequential form and, beside it on every document, the per-byte form the
// kernels run (reflow_amd/csrc/unmarshal_flat.cpp with
// RF_UNMARSHAL_CHECK_TILED), against hand-written bytes, random trees written
// through json_emit.h, and single-byte mutations.  No library, no device; built plain and under
// AddressSanitizer + UBSan (reflow_amd/csrc/Makefile json_parse_test, run by
// tests/test_unmarshal_flat.py).  Every document lives in a heap block of
// exactly its length, so a read past its end is a sanitizer report.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "json_parse.h"
#include "reflow_hip.h"
#include "unmarshal_flat.h"

static int g_fail = 0;
#define CHECK(c)                                                \
    do {                                                        \
        if (!(c)) {                                             \
            printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
            ++g_fail;                                           \
        }                                                       \
    } while (0)

using rf::HostForest;
enum { ST = 1, STR = 2, IDB = 4, SZ = 8, ORD = 16, DEP = 32, LEN = 64 };

// one document, in a block of exactly its length, through both forms
static uint32_t run(const std::string& doc, HostForest* f) {
    std::unique_ptr<uint8_t[]> block(new uint8_t[doc.size() ? doc.size() : 1]);
    if (!doc.empty()) memcpy(block.get(), doc.data(), doc.size());
    const uint64_t offs[2] = {0, doc.size()};
    const int rc = rf::unmarshal_flat(block.get(), offs, 1, RF_UNMARSHAL_CHECK_TILED, 1, f);
    if (rc != RF_OK) {
        printf("  the forms disagree on: %.200s\n  %s\n", doc.c_str(), rf_last_error());
        ++g_fail;
        return ~0u;
    }
    CHECK((f->status[0] == RF_OK) == (f->reason[0] == 0));
    return f->reason[0];
}
static uint32_t why(const std::string& doc) {
    HostForest f;
    return run(doc, &f);
}

static const std::string HEX1 = "0102030405060708090a0b0c0d0e0f101112131415161718191a1b1c1d1e1f20";
static std::string ent(const std::string& quoted_path, const std::string& size, const std::string& hex = HEX1) {
    return quoted_path + ":{\"ID\":\"sha256:" + hex + "\",\"Size\":" + size + "}";
}
static std::string one(const std::string& quoted_path, const std::string& size = "1") {
    return "{\"Fileset\":{" + ent(quoted_path, size) + "}}";
}

static void hand_cases() {
    HostForest f;
    CHECK(run("{}", &f) == 0 && f.n_nodes == 1 && f.n_entries == 0 && f.node_depth[0] == 0);
    CHECK(run(one("\"a\"", "7"), &f) == 0 && f.n_entries == 1 && f.sizes[0] == 7 && f.paths[0] == 'a' &&
          f.path_off[1] == 1 && f.ids32[0] == 1 && f.ids32[31] == 32);
    CHECK(run("{\"List\":[{}]}", &f) == 0 && f.n_nodes == 2 && f.node_depth[0] == 1 && f.node_depth[1] == 0);
    CHECK(run("{\"List\":[{}],\"Fileset\":{" + ent("\"b\"", "-2") + "}}", &f) == 0 && f.n_nodes == 2 &&
          f.entry_ptr[1] == 0 && f.entry_ptr[2] == 1 && f.sizes[0] == -2);
    CHECK(run("{\"Fileset\":{" + ent("\"B\"", "0") + "," + ent("\"a/b\"", "0") + "," + ent("\"b\"", "0") + "}}", &f) == 0 &&
          f.n_entries == 3 && f.path_off[3] == 5);
    CHECK(run("{\"List\":[{\"Fileset\":{" + ent("\"x\"", "1") + "}},{\"List\":[{},{}]}],\"Fileset\":{" + ent("\"y\"", "2") +
                  "}}",
              &f) == 0 &&
          f.n_nodes == 5 && f.n_entries == 2 && f.entry_ptr[1] == 1 && f.entry_ptr[4] == 1 && f.entry_ptr[5] == 2 &&
          f.node_depth[1] == 2 && f.node_depth[3] == 1 && f.node_depth[4] == 0);
    // strings, read backwards
    const struct {
        std::string want, in;
    } strings[] = {
        {"plain/path.fq", "\"plain/path.fq\""},
        {"a\"b\\c", "\"a\\\"b\\\\c\""},
        {"\n\r\t", "\"\\n\\r\\t\""},
        {std::string("\x00\x08\x0c\x1f", 4), "\"\\u0000\\u0008\\u000c\\u001f\""},
        {"<>&", "\"\\u003c\\u003e\\u0026\""},
        {"\x7f", "\"\x7f\""},
        {"\xc3\xa9\xe6\x97\xa5\xf0\x9f\x98\x80", "\"\xc3\xa9\xe6\x97\xa5\xf0\x9f\x98\x80\""},
        {"\xe2\x80\xa8\xe2\x80\xa9", "\"\\u2028\\u2029\""},
        {"\xef\xbf\xbd", "\"\\ufffd\""},
        {"\xef\xbf\xbd\xef\xbf\xbd", "\"\\ufffd\\ufffd\""},
        {"\xef\xbf\xbd", "\"\xef\xbf\xbd\""},
        {"", "\"\""},
    };
    for (const auto& s : strings) {
        CHECK(run(one(s.in), &f) == 0);
        CHECK(f.path_bytes == s.want.size() && memcmp(f.paths.data(), s.want.data(), s.want.size()) == 0);
    }
    for (int64_t v : {(int64_t)0, (int64_t)-1, INT64_MAX, INT64_MIN, (int64_t)10, (int64_t)-10, (int64_t)99}) {
        CHECK(run(one("\"s\"", std::to_string((long long)v)), &f) == 0);
        CHECK(f.sizes[0] == v);
    }
}

static void refusals() {
    CHECK(why("") == LEN);
    CHECK(why("{} ") == ST && why(" {}") == ST && why("{ }") == ST && why("{}}") == ST && why("}}}}") == ST);
    CHECK(why("{\"List\":[]}") == ST && why("{\"Fileset\":{}}") == ST && why("{\"List\":[{}}}") == ST);
    CHECK(why("{\"List\":[{}]]") == ST);
    CHECK(why("{\"Fileset\":{\"a\":{\"Id\":\"sha256:" + HEX1 + "\",\"Size\":1}}}") == ST);
    CHECK(why("{\"Fileset\":{" + ent("\"a\"", "1") + "},\"List\":[{}]}") == ST);
    CHECK(why("{\"Fileset\":{" + ent("\"a\"", "1") + "},\"X\":1}") == ST);
    CHECK(why("{\"Fileset\":{" + ent("\"a\"", "1") + "," + ent("\"a\"", "1") + "}}") == ORD);
    CHECK(why("{\"Fileset\":{" + ent("\"b\"", "1") + "," + ent("\"a\"", "1") + "}}") == ORD);
    CHECK(why("{\"Fileset\":{" + ent("\"a\"", "1") + "," + ent("\"a\\u0000\"", "1") + "}}") == 0);
    for (const char* s : {"\"\\u0041\"", "\"\\u003C\"", "\"\\/\"", "\"<\"", "\"\x01\"", "\"\xff\"", "\"\xe2\x82\"",
                          "\"\xe2\x80\xa8\"", "\"\\b\"", "\"\\u007f\"", "\"\\u0022\"", "\"\\u000a\""})
        CHECK(why(one(s)) == STR);
    CHECK(why("{\"Fileset\":{" + ent("\"a\"", "1", HEX1.substr(1)) + "}}") == IDB);
    CHECK(why("{\"Fileset\":{" + ent("\"a\"", "1", HEX1 + "0") + "}}") == IDB);
    CHECK(why("{\"Fileset\":{" + ent("\"a\"", "1", "0A" + HEX1.substr(2)) + "}}") == IDB);
    CHECK(why("{\"Fileset\":{" + ent("\"a\"", "1", std::string(64, '0')) + "}}") == IDB);
    CHECK(why("{\"Fileset\":{\"a\":{\"ID\":\"sha512:" + HEX1 + "\",\"Size\":1}}}") == IDB);
    for (const char* s : {"-0", "01", "1.0", "1e3", "", "9223372036854775808", "-9223372036854775809", "-", "+1"})
        CHECK(why(one("\"a\"", s)) == SZ);
    CHECK(why(one("\"a\"", "-9223372036854775808")) == 0 && why(one("\"a\"", "9223372036854775807")) == 0);
    // depth: a root at 0, the deepest node allowed at 4096
    for (int deep : {4096, 4097}) {
        std::string d;
        for (int k = 0; k < deep; ++k) d += "{\"List\":[";
        d += "{}";
        for (int k = 0; k < deep; ++k) d += "]}";
        CHECK(why(d) == (deep == 4096 ? 0u : (uint32_t)DEP));
    }
    // documents that end in a backslash run, inside an escape, inside a UTF-8 sequence
    CHECK(why("{\"Fileset\":{\"a\\\\\\") == LEN && why("{\"Fileset\":{\"a\\\\") == LEN);
    CHECK(why("{\"Fileset\":{\"a\\u00") == LEN && why("{\"Fileset\":{\"a\xe6\x97") == STR);
    const std::string full = "{\"List\":[{}],\"Fileset\":{" + ent("\"a\\\\\"", "12") + "," + ent("\"b\"", "-3") + "}}";
    CHECK(why(full) == 0);
    for (size_t k = 0; k < full.size(); ++k) CHECK(why(full.substr(0, k)) != 0);
}

// single-byte mutations of small documents: the two forms must agree on each
static void mutations() {
    std::vector<std::string> docs = {
        "{}",
        "{\"List\":[{}]}",
        "{\"List\":[{},{}]}",
        one("\"a\""),
        one("\"a\\\"b\\\\\"", "-10"),
        one("\"\\u003c\xc3\xa9\"", "0"),
        "{\"List\":[{}],\"Fileset\":{" + ent("\"ID\"", "1") + "," + ent("\"Size\"", "2") + "}}",
        "{\"List\":[{\"Fileset\":{" + ent("\"Fileset\"", "5") + "}},{\"List\":[{}]}]}",
        "{\"Fileset\":{" + ent("\"List\"", "1") + "," + ent("\"a\"", "22") + "," + ent("\"b\"", "333") + "}}",
    };
    const std::string subs = "\"\\{}[],:0a ";
    std::mt19937_64 g(0xD0C);
    uint64_t accepted = 0, refused = 0;
    for (const std::string& d : docs) {
        CHECK(why(d) == 0);
        for (size_t k = 0; k < d.size(); ++k) {
            std::string m = d;
            m.erase(k, 1);
            (why(m) ? refused : accepted)++;
            for (char c : subs) {
                m = d;
                m[k] = c;
                (why(m) ? refused : accepted)++;
            }
            m = d;  // and a random byte, a random insertion
            m[k] = (char)(g() % 256);
            (why(m) ? refused : accepted)++;
            m = d;
            m.insert(k, 1, subs[g() % subs.size()]);
            (why(m) ? refused : accepted)++;
        }
    }
    CHECK(accepted > 0 && refused > 0);
    printf("mutations: %llu accepted, %llu refused\n", (unsigned long long)accepted, (unsigned long long)refused);
}

// random trees, written by this file's own emitter over json_emit.h, read back
struct Node {
    std::vector<Node> kids;
    std::vector<std::pair<std::string, int64_t>> ents;  // sorted, distinct
};
static Node random_node(std::mt19937_64& g, int depth) {
    static const char* pieces[] = {"a", "/", "\"", "\\", "\n", "<", "\xc3\xa9", "\xe6\x97\xa5", "\xe2\x80\xa8",
                                   "\xf0\x9f\x98\x80", "\x01", "\x7f", "z", "\xef\xbf\xbd", "&", "\t"};
    Node n;
    if (depth < 3 && g() % 10 < 4)
        for (int k = (int)(g() % 4); k > 0; --k) n.kids.push_back(random_node(g, depth + 1));
    if (g() % 10 < 8)
        for (int m = (int)(g() % 7); m > 0; --m) {
            std::string p;
            for (int k = (int)(g() % 9); k > 0; --k) p += pieces[g() % 16];
            n.ents.push_back({p, (int64_t)g()});
        }
    std::sort(n.ents.begin(), n.ents.end());
    n.ents.erase(std::unique(n.ents.begin(), n.ents.end(), [](auto& a, auto& b) { return a.first == b.first; }),
                 n.ents.end());
    return n;
}
static void emit(const Node& n, std::string* o, uint64_t* nodes, uint64_t* ents) {
    *o += "{";
    if (!n.kids.empty()) {
        *o += "\"List\":[";
        for (size_t k = 0; k < n.kids.size(); ++k) {
            if (k) *o += ",";
            emit(n.kids[k], o, nodes, ents);
        }
        *o += "]";
    }
    if (!n.ents.empty()) {
        if (!n.kids.empty()) *o += ",";
        *o += "\"Fileset\":{";
        uint8_t id[32];
        for (int k = 0; k < 32; ++k) id[k] = (uint8_t)(k + 1);
        for (size_t k = 0; k < n.ents.size(); ++k) {
            const auto& e = n.ents[k];
            const auto* p = reinterpret_cast<const uint8_t*>(e.first.data());
            std::string buf(rf::json::entry_len(p, (uint32_t)e.first.size(), e.second) + 1, '\0');
            uint8_t* end = rf::json::emit_entry(reinterpret_cast<uint8_t*>(&buf[0]), p, (uint32_t)e.first.size(), id,
                                                e.second, k > 0);
            o->append(buf.data(), (size_t)(end - reinterpret_cast<uint8_t*>(&buf[0])));
            ++*ents;
        }
        *o += "}";
    }
    *o += "}";
    ++*nodes;
}
static void check_values(const Node& n, const HostForest& f, uint64_t* node, uint64_t* entry, uint32_t depth) {
    for (const Node& k : n.kids) check_values(k, f, node, entry, depth + 1);
    CHECK(f.node_depth[*node] == depth && f.entry_ptr[*node] == *entry);
    for (const auto& e : n.ents) {
        const uint64_t b = f.path_off[*entry], l = f.path_off[*entry + 1] - b;
        CHECK(l == e.first.size() && memcmp(f.paths.data() + b, e.first.data(), l) == 0 && f.sizes[*entry] == e.second);
        ++*entry;
    }
    ++*node;
    CHECK(f.entry_ptr[*node] == *entry);
}

static void round_trips() {
    std::mt19937_64 g(0xB0B);
    std::string all;
    std::vector<uint64_t> offs{0};
    std::vector<Node> trees;
    uint64_t nodes = 0, ents = 0;
    for (int i = 0; i < 300; ++i) {
        trees.push_back(random_node(g, 0));
        emit(trees.back(), &all, &nodes, &ents);
        offs.push_back(all.size());
    }
    std::unique_ptr<uint8_t[]> block(new uint8_t[all.size()]);
    memcpy(block.get(), all.data(), all.size());
    for (unsigned threads : {1u, 4u}) {
        HostForest f;
        CHECK(rf::unmarshal_flat(block.get(), offs.data(), trees.size(), RF_UNMARSHAL_CHECK_TILED, threads, &f) == RF_OK);
        CHECK(f.n_accepted == trees.size() && f.n_nodes == nodes && f.n_entries == ents);
        uint64_t node = 0, entry = 0;
        for (size_t i = 0; i < trees.size() && f.n_accepted == trees.size(); ++i) {
            CHECK(f.doc_node_ptr[i] == node);
            check_values(trees[i], f, &node, &entry, 0);
        }
        // the List CSR from the closing order
        std::vector<uint64_t> lp(f.n_nodes + 1);
        std::vector<uint32_t> lc(f.n_nodes + 1), roots(trees.size());
        CHECK(rf_fileset_forest_tree(f.doc_node_ptr.data(), trees.size(), f.node_depth.data(), f.n_nodes, lp.data(),
                                     lc.data(), roots.data()) == RF_OK);
        CHECK(lp[f.n_nodes] == f.n_nodes - trees.size());
        for (size_t i = 0; i < trees.size(); ++i) CHECK(roots[i] + 1 == f.doc_node_ptr[i + 1]);
    }
}

int main() {
    hand_cases();
    refusals();
    mutations();
    round_trips();
    if (g_fail) {
        printf("%d checks failed\n", g_fail);
        return 1;
    }
    printf("PASS\n");
    return 0;
}
