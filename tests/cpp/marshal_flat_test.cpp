// marshal_flat_test.cpp -- the Fileset values' piece stream on the host:
// reflow_amd/csrc/marshal_flat.cpp (flatten, sort, execute) over json_emit.h,
// the per-piece code the marshal kernels run, against wire.cpp's recursive
// marshaller and hand-written bytes.  No library, no device; built plain and
// under AddressSanitizer + UBSan (reflow_amd/csrc/Makefile marshal_flat_test,
// run by tests/test_marshal_flat.py).  Every path lives in a heap block of
// exactly its length, so a read past a path's end is a sanitizer report.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <memory>
#include <random>
#include <string>
#include <vector>

#include "json_emit.h"
#include "marshal_flat.h"
#include "reflow_hip.h"

static int g_fail = 0;
#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);    \
            ++g_fail;                                              \
        }                                                          \
    } while (0)

struct Tree {
    std::vector<uint64_t> list_ptr{0}, entry_ptr{0};
    std::vector<uint32_t> list_child;
    std::vector<std::unique_ptr<char[]>> store;
    std::vector<const char*> paths;
    std::vector<uint32_t> path_lens;
    std::vector<uint8_t> ids;
    std::vector<int64_t> sizes;
    // node i's children are given when it is added; entries are added first
    void entry(const std::string& p, uint8_t idb, int64_t size) {
        std::unique_ptr<char[]> b(new char[p.size() ? p.size() : 1]);
        if (!p.empty()) memcpy(b.get(), p.data(), p.size());
        paths.push_back(b.get());
        store.push_back(std::move(b));
        path_lens.push_back((uint32_t)p.size());
        for (int k = 0; k < 32; ++k) ids.push_back((uint8_t)(idb + k));
        sizes.push_back(size);
    }
    uint32_t node(const std::vector<uint32_t>& kids) {  // closes the entries added since the last node
        for (uint32_t k : kids) list_child.push_back(k);
        list_ptr.push_back(list_child.size());
        entry_ptr.push_back(paths.size());
        return (uint32_t)list_ptr.size() - 2;
    }
    rf_fileset_tree c() const {
        rf_fileset_tree t{};
        t.n_nodes = list_ptr.size() - 1;
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

static std::string reference(const rf_fileset_tree& t, uint32_t root, int* rc_out = nullptr) {
    uint64_t need = 0;
    int rc = rf_fileset_marshal_json(&t, root, nullptr, 0, &need);
    if (rc != RF_OK && need == 0) {
        if (rc_out) *rc_out = rc;
        return std::string();
    }
    std::string o(need, '\0');
    rc = rf_fileset_marshal_json(&t, root, reinterpret_cast<uint8_t*>(&o[0]), need, &need);
    if (rc_out) *rc_out = rc;
    return o;
}

// every root in one call: equal to the reference per value, offs consistent
static void compare_all(const Tree& tr, const std::vector<uint32_t>& roots) {
    const rf_fileset_tree t = tr.c();
    std::vector<uint64_t> offs(roots.size() + 1, ~0ull);
    uint64_t need = 0;
    int rc = rf_fileset_marshal_flat(&t, roots.data(), roots.size(), nullptr, 0, offs.data(), &need);
    CHECK(rc == (need ? RF_EINVAL : RF_OK));
    std::unique_ptr<uint8_t[]> out(new uint8_t[need ? need : 1]);  // exactly the bytes needed
    rc = rf_fileset_marshal_flat(&t, roots.data(), roots.size(), out.get(), need, offs.data(), &need);
    CHECK(rc == RF_OK);
    if (rc != RF_OK) {
        printf("  %s\n", rf_last_error());
        return;
    }
    CHECK(offs[0] == 0 && offs[roots.size()] == need);
    for (size_t i = 0; i < roots.size(); ++i) {
        const std::string want = reference(t, roots[i]);
        CHECK(offs[i + 1] - offs[i] == want.size());
        if (offs[i + 1] - offs[i] == want.size()) CHECK(memcmp(out.get() + offs[i], want.data(), want.size()) == 0);
    }
}

static std::string hex_of(uint8_t idb) {
    static const char* H = "0123456789abcdef";
    std::string s;
    for (int k = 0; k < 32; ++k) {
        const uint8_t b = (uint8_t)(idb + k);
        s.push_back(H[b >> 4]);
        s.push_back(H[b & 15]);
    }
    return s;
}

static std::string flat_one(const Tree& tr, uint32_t root) {
    const rf_fileset_tree t = tr.c();
    uint64_t need = 0, offs[2];
    rf_fileset_marshal_flat(&t, &root, 1, nullptr, 0, offs, &need);
    std::string o(need, '\0');
    const int rc = rf_fileset_marshal_flat(&t, &root, 1, reinterpret_cast<uint8_t*>(&o[0]), need, offs, &need);
    CHECK(rc == RF_OK);
    return o;
}

static void hand_cases() {
    const std::string id = "{\"ID\":\"sha256:" + hex_of(1) + "\",\"Size\":";
    {
        Tree t;
        const uint32_t r = t.node({});
        CHECK(flat_one(t, r) == "{}");
    }
    {
        Tree t;
        t.entry("a", 1, 7);
        const uint32_t r = t.node({});
        CHECK(flat_one(t, r) == "{\"Fileset\":{\"a\":" + id + "7}}}");
    }
    {
        Tree t;
        const uint32_t e = t.node({});
        t.entry("b", 1, -2);
        const uint32_t r = t.node({e});
        CHECK(flat_one(t, e) == "{}");
        CHECK(flat_one(t, r) == "{\"List\":[{}],\"Fileset\":{\"b\":" + id + "-2}}}");
        const uint32_t l = t.node({e, e});
        CHECK(flat_one(t, l) == "{\"List\":[{},{}]}");
        compare_all(t, {r, e, l, r});
    }
    {
        Tree t;
        t.entry("b", 1, 0);
        t.entry("B", 1, 0);
        t.entry("a/b", 1, 0);
        const uint32_t r = t.node({});
        CHECK(flat_one(t, r) == "{\"Fileset\":{\"B\":" + id + "0},\"a/b\":" + id + "0},\"b\":" + id + "0}}}");
    }
    // escaping: Go 1.9/1.10 encodeState.string with escapeHTML
    const struct {
        std::string in, want;
    } strings[] = {
        {"plain/path.fq", "\"plain/path.fq\""},
        {"a\"b\\c", "\"a\\\"b\\\\c\""},
        {"\n\r\t", "\"\\n\\r\\t\""},
        {std::string("\x00\x08\x0c\x1f", 4), "\"\\u0000\\u0008\\u000c\\u001f\""},
        {"<>&", "\"\\u003c\\u003e\\u0026\""},
        {"\x7f", "\"\x7f\""},
        {"\xc3\xa9\xe6\x97\xa5\xf0\x9f\x98\x80", "\"\xc3\xa9\xe6\x97\xa5\xf0\x9f\x98\x80\""},
        {"\xe2\x80\xa8\xe2\x80\xa9", "\"\\u2028\\u2029\""},
        {"\xff", "\"\\ufffd\""},
        {"\xe2\x82", "\"\\ufffd\\ufffd\""},
        {"\xed\xa0\x80", "\"\\ufffd\\ufffd\\ufffd\""},
        {"\xc0\xaf", "\"\\ufffd\\ufffd\""},
        {"\xf4\x90\x80\x80", "\"\\ufffd\\ufffd\\ufffd\\ufffd\""},
        {"\xef\xbf\xbd", "\"\xef\xbf\xbd\""},
        {"", "\"\""},
    };
    for (const auto& s : strings) {
        Tree t;
        t.entry(s.in, 1, 1);
        const uint32_t r = t.node({});
        CHECK(flat_one(t, r) == "{\"Fileset\":{" + s.want + ":" + id + "1}}}");
    }
    // sizes across int64
    for (int64_t v : {(int64_t)0, (int64_t)-1, INT64_MAX, INT64_MIN, (int64_t)10, (int64_t)-10, (int64_t)99}) {
        Tree t;
        t.entry("s", 1, v);
        const uint32_t r = t.node({});
        CHECK(flat_one(t, r) == "{\"Fileset\":{\"s\":" + id + std::to_string((long long)v) + "}}}");
    }
}

// A path that ends inside a multi-byte sequence, followed IN ONE BLOB by a path
// that begins with the continuation byte that would complete it: the sequence
// bound is the path's own end.
static void adjacent_paths() {
    static const char blob[] = "\xe2\x82\xac";
    rf_fileset_tree t{};
    const uint64_t list_ptr[2] = {0, 0}, entry_ptr[2] = {0, 2};
    const char* paths[2] = {blob, blob + 2};
    const uint32_t lens[2] = {2, 1};
    uint8_t ids[64];
    for (int k = 0; k < 64; ++k) ids[k] = (uint8_t)(1 + k % 32);
    const int64_t sizes[2] = {1, 2};
    t.n_nodes = 1;
    t.list_ptr = list_ptr;
    t.entry_ptr = entry_ptr;
    t.paths = paths;
    t.path_lens = lens;
    t.ids32 = ids;
    t.sizes = sizes;
    const uint32_t root = 0;
    uint64_t need = 0, offs[2];
    rf_fileset_marshal_flat(&t, &root, 1, nullptr, 0, offs, &need);
    std::string o(need, '\0');
    CHECK(rf_fileset_marshal_flat(&t, &root, 1, reinterpret_cast<uint8_t*>(&o[0]), need, offs, &need) == RF_OK);
    const std::string id = "{\"ID\":\"sha256:" + hex_of(1) + "\",\"Size\":";
    // bytewise order: "\xac" < "\xe2\x82"
    CHECK(o == "{\"Fileset\":{\"\\ufffd\":" + id + "2},\"\\ufffd\\ufffd\":" + id + "1}}}");
    CHECK(o == reference(t, 0));
    // the primitives on the blob itself, bounded to the first path
    CHECK(rf::json::utf8_seq(reinterpret_cast<const uint8_t*>(blob), 2, 0) == 0);
    CHECK(rf::json::utf8_seq(reinterpret_cast<const uint8_t*>(blob), 3, 0) == 3);
    CHECK(rf::json::string_len(reinterpret_cast<const uint8_t*>(blob), 2) == 14);
}

static std::string random_path(std::mt19937_64& g, bool raw) {
    static const char* multi[] = {"\xc3\xa9", "\xe6\x97\xa5", "\xe2\x80\xa8", "\xf0\x9f\x98\x80"};
    std::string p;
    const int n = (int)(g() % (raw ? 40 : 13));
    for (int i = 0; i < n; ++i) p.push_back((char)(g() % 256));
    if (g() % 10 < 3) p += multi[g() % 4];
    if (raw && g() % 4 == 0 && !p.empty()) {  // end inside a sequence
        p.push_back((char)(0xE0 + g() % 16));
        if (g() % 2) p.push_back((char)(0x80 + g() % 64));
    }
    return p;
}

static uint32_t random_tree(std::mt19937_64& g, Tree& t, int depth, bool raw) {
    std::vector<uint32_t> kids;
    if (depth < 3 && g() % 10 < 4) {
        const int k = (int)(g() % 4);
        for (int i = 0; i < k; ++i) kids.push_back(random_tree(g, t, depth + 1, raw));
    }
    // a node's entries must be contiguous: its children are complete by now
    if (g() % 10 < 8) {
        std::vector<std::string> seen;
        const int m = (int)(g() % 7);
        for (int i = 0; i < m; ++i) {
            std::string p = random_path(g, raw);
            bool dup = false;
            for (const std::string& q : seen) dup |= q == p;
            if (dup) continue;
            seen.push_back(p);
            t.entry(p, (uint8_t)(1 + g() % 200), (int64_t)g());
        }
    }
    return t.node(kids);
}

static void random_cases() {
    std::mt19937_64 g(0xB0B);
    for (int round = 0; round < 60; ++round) {
        Tree t;
        std::vector<uint32_t> roots;
        for (int i = 0; i < 5; ++i) roots.push_back(random_tree(g, t, 0, round >= 30));
        if (round % 3 == 0) roots.push_back(roots[0]);  // a root listed twice
        compare_all(t, roots);
    }
    // one large Map: sorted input is left alone, shuffled input goes through the threaded sort
    for (int shuffled = 0; shuffled < 2; ++shuffled) {
        Tree t;
        const int n = 70000;
        std::vector<int> order(n);
        for (int i = 0; i < n; ++i) order[i] = i;
        if (shuffled)
            for (int i = n - 1; i > 0; --i) std::swap(order[i], order[g() % (i + 1)]);
        char buf[32];
        for (int i = 0; i < n; ++i) {
            snprintf(buf, sizeof buf, "d%03d/f%06d", order[i] / 1000, order[i]);
            t.entry(buf, (uint8_t)(1 + i % 100), i);
        }
        const uint32_t r = t.node({});
        const rf_fileset_tree c = t.c();
        rf::FlatPieces f;
        CHECK(rf::fileset_flatten(&c, &r, 1, true, 4, &f) == RF_OK);
        CHECK(f.sorted_groups == (shuffled ? 0u : 1u) && f.unsorted_groups == (shuffled ? 1u : 0u));
        CHECK(f.a.size() == (size_t)n + 2);
        compare_all(t, {r});
    }
}

static void refusals() {
    {  // duplicate keys, adjacent and apart
        Tree t;
        t.entry("x", 1, 1);
        t.entry("x", 1, 2);
        const uint32_t r = t.node({});
        t.entry("b", 1, 1);
        t.entry("a", 1, 1);
        t.entry("b", 1, 1);
        const uint32_t r2 = t.node({});
        const rf_fileset_tree c = t.c();
        uint64_t need = 0;
        CHECK(rf_fileset_marshal_flat(&c, &r, 1, nullptr, 0, nullptr, &need) == RF_EINVAL);
        CHECK(strstr(rf_last_error(), "duplicate") != nullptr);
        CHECK(rf_fileset_marshal_flat(&c, &r2, 1, nullptr, 0, nullptr, &need) == RF_EINVAL);
        int rc = 0;
        reference(c, r, &rc);
        CHECK(rc == RF_EINVAL);
    }
    {  // a zero ID
        Tree t;
        t.entry("a", 1, 1);
        const uint32_t r = t.node({});
        memset(t.ids.data(), 0, 32);
        const rf_fileset_tree c = t.c();
        uint64_t need = 0;
        CHECK(rf_fileset_marshal_flat(&c, &r, 1, nullptr, 0, nullptr, &need) == RF_EINVAL);
        CHECK(strstr(rf_last_error(), "zero file ID") != nullptr);
        rf::FlatPieces f;  // IDs on the device: the host does not look
        CHECK(rf::fileset_flatten(&c, &r, 1, false, 1, &f) == RF_OK);
    }
    {  // a bad root, a cyclic list_child, a CSR that runs backwards
        Tree t;
        const uint32_t r = t.node({0});  // node 0 lists itself
        const rf_fileset_tree c = t.c();
        uint64_t need = 0;
        const uint32_t bad = 7;
        CHECK(rf_fileset_marshal_flat(&c, &bad, 1, nullptr, 0, nullptr, &need) == RF_EINVAL);
        CHECK(rf_fileset_marshal_flat(&c, &r, 1, nullptr, 0, nullptr, &need) == RF_EINVAL);
        CHECK(strstr(rf_last_error(), "4096") != nullptr);
        Tree u;
        u.entry("a", 1, 1);
        u.node({});
        u.node({});
        u.entry_ptr[1] = 1;
        u.entry_ptr[2] = 0;
        const rf_fileset_tree cu = u.c();
        const uint32_t one = 1;
        CHECK(rf_fileset_marshal_flat(&cu, &one, 1, nullptr, 0, nullptr, &need) == RF_EINVAL);
        CHECK(rf_fileset_marshal_flat(nullptr, &one, 1, nullptr, 0, nullptr, &need) == RF_EINVAL);
    }
    {  // a short buffer: the length is reported, nothing is written
        Tree t;
        t.entry("a", 1, 1);
        const uint32_t r = t.node({});
        const rf_fileset_tree c = t.c();
        uint64_t need = 0;
        uint8_t small[4] = {9, 9, 9, 9};
        CHECK(rf_fileset_marshal_flat(&c, &r, 1, small, 4, nullptr, &need) == RF_EINVAL);
        CHECK(need == reference(c, r).size() && small[0] == 9 && small[3] == 9);
    }
}

int main() {
    hand_cases();
    adjacent_paths();
    random_cases();
    refusals();
    if (g_fail) {
        printf("%d checks failed\n", g_fail);
        return 1;
    }
    printf("PASS\n");
    return 0;
}
