// assoc_persist_test.cpp -- the HBM assoc's scan, compaction and save /
// restore through the C++ host mirror (include/reflow_host.hpp), against a
// std::map that restates the in-memory assoc (test/testutil/assoc.go:34-56).
//   TestCountScan   Count / Scan equal the map after puts, overwrites and deletes
//   TestCompact     deleted keys leave the table; Get / Put behave as before
//   TestSaveRestore a saved file restores to the same contents; a damaged one is refused
// Exit status 0 iff every check passes.
#include <unistd.h>

#include <cstdio>
#include <map>
#include <string>
#include <vector>

#include "reflow_host.hpp"

using namespace reflow;

static int failures = 0;
#define EXPECT(cond, ...)                                   \
    do {                                                    \
        if (!(cond)) {                                      \
            ++failures;                                     \
            fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
            fprintf(stderr, __VA_ARGS__);                   \
            fprintf(stderr, "\n");                          \
        }                                                   \
    } while (0)

using Model = std::map<std::pair<int, std::array<uint8_t, 32>>, Digest>;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {  // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static Digest rnd_digest() {
    Digest d;
    for (int i = 0; i < 32; i += 8) {
        const uint64_t x = rnd();
        memcpy(d.b.data() + i, &x, 8);
    }
    d.b[0] |= 1;  // never zero
    return d;
}

static void put(Assoc& a, Model& m, int kind, const std::vector<Digest>& keys, const std::vector<Digest>& vals) {
    const std::vector<int> st = a.PutBatch((AssocKind)kind, {}, keys, vals);
    for (size_t i = 0; i < keys.size(); ++i) {
        EXPECT(st[i] == RF_OK, "put status %d", st[i]);
        if (vals[i].IsZero())
            m.erase({kind, keys[i].b});
        else
            m[{kind, keys[i].b}] = vals[i];
    }
}

static Model as_model(const std::vector<Assoc::Entry>& es) {
    Model m;
    for (const Assoc::Entry& e : es) {
        EXPECT(!m.count({e.kind, e.key.b}), "scan returned a key twice");
        m[{e.kind, e.key.b}] = e.value;
    }
    return m;
}

static Model of_kind(const Model& m, int kind) {
    Model o;
    for (const auto& kv : m)
        if (kv.first.first == kind) o.insert(kv);
    return o;
}

// 3,000 keys over two kinds, a third of them deleted, some overwritten
static void fill(Assoc& a, Model& m, std::vector<Digest>* keys_out) {
    std::vector<Digest> keys(3000), vals(3000);
    for (size_t i = 0; i < keys.size(); ++i) keys[i] = rnd_digest(), vals[i] = rnd_digest();
    for (int kind = 0; kind < 2; ++kind) {
        put(a, m, kind, keys, vals);
        std::vector<Digest> dk, dv;
        for (size_t i = kind; i < keys.size(); i += 3) dk.push_back(keys[i]), dv.push_back(Digest{});
        put(a, m, kind, dk, dv);
        std::vector<Digest> ok(keys.begin(), keys.begin() + 100), ov;
        for (size_t i = 0; i < ok.size(); ++i) ov.push_back(rnd_digest());
        put(a, m, kind, ok, ov);
    }
    if (keys_out) *keys_out = keys;
}

static void TestCountScan(Engine& e) {
    Assoc a(e, 16);
    EXPECT(a.Scan().empty() && a.Count().first == 0 && a.Count().second == 0, "an empty table scans empty");
    Model m;
    fill(a, m, nullptr);
    EXPECT(as_model(a.Scan()) == m, "scan of every kind differs from the model");
    for (int kind = 0; kind < 2; ++kind) {
        EXPECT(as_model(a.Scan(kind)) == of_kind(m, kind), "scan of kind %d differs from the model", kind);
        EXPECT(a.Count(kind).first == of_kind(m, kind).size(), "count of kind %d", kind);
    }
    const auto c = a.Count();
    EXPECT(c.first == m.size() && c.first + c.second == a.Stats().first, "live %llu deleted %llu occupied %llu",
           (unsigned long long)c.first, (unsigned long long)c.second, (unsigned long long)a.Stats().first);
    EXPECT(a.Scan(7).empty(), "a kind nobody used scans empty");
}

static void check_gets(Assoc& a, const Model& m, const std::vector<Digest>& keys) {
    for (int kind = 0; kind < 2; ++kind) {
        const auto got = a.GetBatch((AssocKind)kind, keys);
        for (size_t i = 0; i < keys.size(); ++i) {
            const auto it = m.find({kind, keys[i].b});
            EXPECT(got[i].has_value() == (it != m.end()) && (!got[i] || *got[i] == it->second), "get kind %d key %zu",
                   kind, i);
        }
    }
}

static void TestCompact(Engine& e) {
    Assoc a(e, 16);
    Model m;
    std::vector<Digest> keys;
    fill(a, m, &keys);
    EXPECT(a.Count().second > 0, "the fill deletes keys");
    a.Compact();
    EXPECT(a.Stats().first == m.size() && a.Count().second == 0, "occupied %llu after compaction, live %zu",
           (unsigned long long)a.Stats().first, m.size());
    EXPECT(a.Stats().second == 8192, "capacity %llu for %zu live keys", (unsigned long long)a.Stats().second, m.size());
    check_gets(a, m, keys);
    // a compare-and-set on a key that compaction dropped: the value is still "none"
    bool refused = false;
    try {
        a.Put(AssocFileset, rnd_digest(), keys[300], rnd_digest());  // keys[300] was deleted in kind 0
    } catch (const Error& err) {
        refused = err.code == RF_EPRECONDITION;
    }
    EXPECT(refused, "a compare-and-set on a deleted key must fail its precondition");
    std::vector<Digest> vals(keys.size());
    for (Digest& v : vals) v = rnd_digest();
    put(a, m, 0, keys, vals);  // re-inserts the deleted third
    check_gets(a, m, keys);
    a.Compact(50000);
    EXPECT(a.Stats().second == 131072, "capacity %llu for min_capacity 50000", (unsigned long long)a.Stats().second);
    check_gets(a, m, keys);
}

static void TestSaveRestore(Engine& e) {
    const std::string path = "/tmp/assoc_persist_test." + std::to_string((long)getpid()) + ".bin";
    Assoc a(e, 16);
    Model m;
    std::vector<Digest> keys;
    fill(a, m, &keys);
    a.Save(path);
    {
        std::unique_ptr<Assoc> b = Assoc::Restore(e, path);
        EXPECT(as_model(b->Scan()) == m, "the restored table differs from the saved one");
        EXPECT(b->Stats().first == m.size() && b->Stats().second == 8192, "restored occupied %llu capacity %llu",
               (unsigned long long)b->Stats().first, (unsigned long long)b->Stats().second);
        check_gets(*b, m, keys);
        Model mb = m;
        std::vector<Digest> vals(keys.size());
        for (Digest& v : vals) v = rnd_digest();
        put(*b, mb, 1, keys, vals);
        check_gets(*b, mb, keys);
    }
    // one flipped bit in an entry: refused, and the engine goes on working
    FILE* f = fopen(path.c_str(), "r+b");
    EXPECT(f != nullptr, "cannot reopen %s", path.c_str());
    if (f) {
        fseek(f, 64 + 68 * 5 + 40, SEEK_SET);
        int c = fgetc(f);
        fseek(f, -1, SEEK_CUR);
        fputc(c ^ 0x10, f);
        fclose(f);
        int code = RF_OK;
        try {
            Assoc::Restore(e, path);
        } catch (const Error& err) {
            code = err.code;
        }
        EXPECT(code == RF_EINTEGRITY, "a damaged file restored with code %d", code);
        check_gets(a, m, keys);
    }
    unlink(path.c_str());
}

int main() {
    try {
        Engine e(0);
        TestCountScan(e);
        TestCompact(e);
        TestSaveRestore(e);
    } catch (const std::exception& ex) {
        fprintf(stderr, "exception: %s\n", ex.what());
        return 2;
    }
    if (failures) {
        fprintf(stderr, "%d failure(s)\n", failures);
        return 1;
    }
    printf("PASS\n");
    return 0;
}
