// phys_mirror_test.cpp -- reflow::PhysicalKeys (include/reflow_host.hpp) on the
// device: values set from Fileset objects and from an unmarshalled forest, the
// consumers' keys against SHA-256 of Fileset::WriteDigest's bytes ‖ suffix
// (Flow.PhysicalDigest, flow.go:764-792), the zero digest while a dep has no
// value, a replaced and a cleared value, and the value digests against
// FilesetDigests.  Linked against the library; run by
// tests/test_gpu_physkeys_host.py.
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

static File file(uint8_t seed, int64_t size) {
    File f;
    for (size_t k = 0; k < f.ID.b.size(); ++k) f.ID.b[k] = (uint8_t)(seed + k);
    f.Size = size;
    return f;
}

static std::string material(const Fileset& v) {
    std::string w;
    v.WriteDigest(w);
    return w;
}

int main() {
    try {
        Engine e(0);
        Digester dg(e);
        Fileset leaf, empty, mid, wide;
        leaf.Map["a/b.bam"] = file(1, 7);
        leaf.Map["quote\"back\\slash\n<&>"] = file(2, -3);
        leaf.Map[""] = file(3, 1);
        mid.List.emplace(std::vector<Fileset>{leaf, empty});
        mid.Map["ignored: the List wins"] = file(4, 9);
        for (int i = 0; i < 3000; ++i) wide.Map["d" + std::to_string(i % 7) + "/f" + std::to_string(i)] = file((uint8_t)(1 + i % 200), i);
        // nodes 0..3 are sources; 4 = extern(0), 5 = exec(1, 2, 1), 6 = exec(3, 0), 7 = extern() without deps
        const std::vector<uint64_t> dep_ptr = {0, 0, 0, 0, 0, 1, 4, 6, 6};
        const std::vector<uint32_t> deps = {0, 1, 2, 1, 3, 0};
        const uint64_t no = PhysicalKeys::NoRow;
        const std::vector<uint64_t> phys_row = {no, no, no, no, 2, 0, 3, 1};
        const std::vector<std::string> suffixes = {"", "", "", "", "s3://bucket/out", std::string("image\0cmd", 9) + std::string(8, '\1'),
                                                   "", "url"};
        PhysicalKeys pk(e, dep_ptr, deps, phys_row, suffixes);
        std::vector<Digest> keys(5);
        for (Digest& k : keys) k.b.fill(0x77);
        const Digest untouched = keys[4], zero{};

        // values 0 and 1 from objects, 2 and 3 through JSON and the device unmarshal
        pk.SetValues({0, 1}, std::vector<const Fileset*>{&leaf, &mid});
        auto r = pk.Update({0, 1}, RF_PHYS_CONSUMERS, keys);
        CHECK(r.affected == 3 && r.written == 1 && r.zeroed == 2);
        CHECK((r.nodes == std::vector<uint32_t>{4, 5, 6}) && (r.computable == std::vector<uint8_t>{1, 0, 0}));
        CHECK(keys[2].b == dg.FromBytes(material(leaf) + suffixes[4]).b);
        CHECK(keys[0].b == zero.b && keys[3].b == zero.b && keys[1].b == untouched.b && keys[4].b == untouched.b);

        const std::vector<std::string> docs = {MarshalJSON(empty), "{\"Fileset\": {}}", MarshalJSON(wide)};
        std::string all;
        std::vector<uint64_t> offs{0};
        for (const std::string& d : docs) {
            all += d;
            offs.push_back(all.size());
        }
        rf_fileset_forest* f = nullptr;
        Check(rf_fileset_unmarshal(e.ctx(), reinterpret_cast<const uint8_t*>(all.data()), offs.data(), docs.size(), &f, nullptr));
        bool threw = false;
        try {
            pk.SetValues({2, 1, 3}, f);  // the middle document is not canonical: refused, nothing changes
        } catch (const Error&) {
            threw = true;
        }
        CHECK(threw && pk.Stats().n_values == 2);
        pk.SetValues({2, 0xffffffffu, 3}, f);
        rf_fileset_forest_free(f);
        r = pk.Update({2, 3}, RF_PHYS_CONSUMERS | RF_PHYS_SELF, keys);
        CHECK(r.affected == 2 && r.written == 2);
        CHECK(keys[0].b == dg.FromBytes(material(mid) + material(empty) + material(mid) + suffixes[5]).b);
        CHECK(keys[3].b == dg.FromBytes(material(wide) + material(leaf)).b);
        r = pk.Update({7}, RF_PHYS_SELF, keys);
        CHECK(r.written == 1 && keys[1].b == dg.FromBytes("url").b && keys[4].b == untouched.b);

        // the stored materials and their digests
        CHECK(pk.ValueMaterial(1) == material(mid) && pk.ValueMaterial(2).empty() && pk.ValueMaterial(3) == material(wide));
        const auto vd = pk.ValueDigests({0, 1, 2, 3});
        const auto want = FilesetDigests(e, {&leaf, &mid, &empty, &wide});
        for (size_t i = 0; i < 4; ++i) CHECK(vd[i].b == want[i].b);

        // replaced, then cleared
        pk.SetValues({0}, std::vector<const Fileset*>{&wide});
        r = pk.Update({0}, RF_PHYS_CONSUMERS, keys);
        CHECK(r.written == 2 && keys[2].b == dg.FromBytes(material(wide) + suffixes[4]).b);
        CHECK(keys[3].b == dg.FromBytes(material(wide) + material(wide)).b && pk.Stats().stale_bytes > 0);
        pk.ClearValues({0});
        r = pk.Update({0}, RF_PHYS_CONSUMERS, keys);
        CHECK(r.zeroed == 2 && keys[2].b == zero.b && keys[3].b == zero.b && pk.Stats().n_values == 3);
    } catch (const std::exception& ex) {
        printf("FAIL exception: %s\n", ex.what());
        return 1;
    }
    if (failures) return 1;
    printf("PASS\n");
    return 0;
}
