// unmarshal_mirror_test.cpp -- reflow::UnmarshalFilesets (include/reflow_host.hpp)
// on the device: MarshalJSON's bytes of nested Filesets come back as equal
// values, and a document that is not canonical comes back as an empty optional
// between two that are.  Linked against the library; run by
// tests/test_gpu_unmarshal_host.py.
#include <stdio.h>

#include <string>
#include <vector>

#include "reflow_host.hpp"

using namespace reflow;

static int failures = 0;
#define CHECK(c)                                                \
    do {                                                        \
        if (!(c)) {                                             \
            printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
            ++failures;                                         \
        }                                                       \
    } while (0)

static bool same(const Fileset& a, const Fileset& b) {
    const size_t na = a.List ? a.List->size() : 0, nb = b.List ? b.List->size() : 0;  // omitempty: nil == empty
    if (na != nb || a.Map.size() != b.Map.size()) return false;
    for (size_t i = 0; i < na; ++i)
        if (!same((*a.List)[i], (*b.List)[i])) return false;
    auto x = a.Map.begin();
    auto y = b.Map.begin();
    for (; x != a.Map.end(); ++x, ++y)
        if (x->first != y->first || x->second.ID.b != y->second.ID.b || x->second.Size != y->second.Size) return false;
    return true;
}

static File file(uint8_t seed, int64_t size) {
    File f;
    for (size_t k = 0; k < f.ID.b.size(); ++k) f.ID.b[k] = (uint8_t)(seed + k);
    f.Size = size;
    return f;
}

int main() {
    try {
        Engine e(0);
        Fileset leaf, empty, mid, root;
        leaf.Map["a/b.bam"] = file(1, 7);
        leaf.Map["quote\"back\\slash\n<&>"] = file(2, -3);
        leaf.Map[std::string("nul\0byte", 8)] = file(3, INT64_MIN);
        mid.List.emplace(std::vector<Fileset>{leaf, empty});
        mid.Map["\xc3\xa9\xe6\x97\xa5\xe2\x80\xa8"] = file(4, INT64_MAX);
        root.List.emplace(std::vector<Fileset>{mid, leaf, empty});
        Fileset wide;
        for (int i = 0; i < 3000; ++i) wide.Map["d" + std::to_string(i % 7) + "/f" + std::to_string(i)] = file((uint8_t)(1 + i % 200), i);
        const std::vector<const Fileset*> values = {&root, &empty, &leaf, &wide, &mid};
        std::vector<std::string> docs;
        for (const Fileset* v : values) docs.push_back(MarshalJSON(*v));
        docs.insert(docs.begin() + 2, "{\"Fileset\": {}}");  // not json.Marshal's bytes
        const auto got = UnmarshalFilesets(e, docs);
        CHECK(got.size() == docs.size());
        if (got.size() == docs.size()) {
            CHECK(!got[2].has_value());
            for (size_t i = 0, v = 0; i < docs.size(); ++i) {
                if (i == 2) continue;
                CHECK(got[i].has_value() && same(*got[i], *values[v]));
                if (got[i]) CHECK(MarshalJSON(*got[i]) == docs[i]);
                ++v;
            }
        }
        CHECK(UnmarshalFilesets(e, {}).empty());
    } catch (const std::exception& ex) {
        printf("FAIL: %s\n", ex.what());
        return 1;
    }
    if (failures) return 1;
    printf("PASS\n");
    return 0;
}
