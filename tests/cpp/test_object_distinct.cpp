// ObjectDistinctMirror: the downcalls of bindings/scala/core/.../gpu/ObjectDistinct.scala in the same
// order, over the C ABI, with B = Long (element = id) so that the C oracle can say what the set must be.
// The replica is rsv_host_values.h's HostValues (scala PriorityQueue tie order), as the Scala class
// holds mutable.PriorityQueue[(B, Long)] and mutable.Set[B].
//   case file: "n k seed twin_bits batch" then the expected set's ids, ascending
//   ids: element i repeats an earlier index with probability 0.3, else is new; the id of index j is
//        a hash twin (hi, hi ^ (lo & (2^twin_bits - 1))) of splitmix(j): Long.hashCode folds to twin_bits
//   g++ -std=c++17 -O2 -I include -I reservoir_amd/csrc tests/cpp/test_object_distinct.cpp -lreservoir_hip
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "reservoir_hip.h"
#include "rsv_host_values.h"

static uint64_t mix(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static int64_t id_at(uint64_t i, uint64_t seed, int bits) {
    const bool rep = i > 0 && mix(i ^ 0xABCDull) % 10 < 3;
    const uint64_t src = rep ? mix(i + 77) % i : i;
    const uint64_t v = mix(src * 0x9E3779B97F4A7C15ull + seed);
    const uint64_t hi = v >> 32;
    return (int64_t)((hi << 32) | ((hi ^ (v & ((1ull << bits) - 1))) & 0xFFFFFFFFull));
}

static int64_t long_hash_code(int64_t v) { return (int64_t)(int32_t)((uint64_t)v ^ ((uint64_t)v >> 32)); }

#define CHECK(call)                                                                               \
    do {                                                                                          \
        rsv_status _s = (call);                                                                   \
        if (_s != RSV_OK) {                                                                       \
            std::printf("%s -> %s: %s\n", #call, rsv_status_string(_s), rsv_last_error());        \
            return false;                                                                         \
        }                                                                                         \
    } while (0)

struct ObjectDistinctMirror {
    rsv_sampler* h = nullptr;
    rsv::HostValues values;
    std::vector<int64_t> elems, hashes;  // the batch buffer: map(x) and hash(map(x))
    std::vector<int64_t> offs, cand_h;
    int64_t batch;
    int64_t candidates = 0;

    bool create(int32_t k, uint64_t seed, int64_t batch_) {
        batch = batch_;
        values.reset(k);
        rsv_config cfg;
        CHECK(rsv_config_init(&cfg));
        cfg.kind = RSV_KIND_DISTINCT;
        cfg.max_sample_size = k;
        cfg.hash_kind = RSV_HASH_PRECOMPUTED;
        cfg.seed = seed;
        CHECK(rsv_create(&cfg, &h));
        return true;
    }
    bool flush() {
        const int64_t n = (int64_t)elems.size();
        if (n == 0) return true;
        int64_t c = 0;
        CHECK(rsv_distinct_candidates(h, hashes.data(), n, RSV_MEM_HOST, &c));
        offs.resize((size_t)std::max<int64_t>(c, 1));
        cand_h.resize((size_t)std::max<int64_t>(c, 1));
        if (rsv_candidates_read(h, offs.data(), cand_h.data(), c) != RSV_OK) {  // try / abort
            (void)rsv_candidates_abort(h);
            return false;
        }
        for (int64_t t = 0; t < c; ++t) {
            if (t > 0 && offs[(size_t)t] <= offs[(size_t)t - 1]) {
                std::printf("offsets not ascending at %lld\n", (long long)t);
                (void)rsv_candidates_abort(h);
                return false;
            }
            values.sample(elems[(size_t)offs[(size_t)t]], cand_h[(size_t)t]);
        }
        CHECK(rsv_candidates_commit(h, values.n, values.max_hash));
        candidates += c;
        elems.clear();
        hashes.clear();
        return true;
    }
    bool sample(int64_t id) {
        elems.push_back(id);
        hashes.push_back(long_hash_code(id));
        return (int64_t)elems.size() < batch || flush();
    }
    bool result(std::vector<int64_t>* out) {
        if (!flush()) return false;
        out->assign(values.he.begin() + 1, values.he.begin() + 1 + values.n);
        rsv_destroy(h);  // single use
        h = nullptr;
        return true;
    }
};

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    long long n, k, seed, bits, batch;
    if (std::fscanf(f, "%lld %lld %lld %lld %lld", &n, &k, &seed, &bits, &batch) != 5) return 2;
    std::vector<int64_t> want;
    for (long long v; std::fscanf(f, "%lld", &v) == 1;) want.push_back(v);
    std::fclose(f);

    ObjectDistinctMirror m;
    if (!m.create((int32_t)k, (uint64_t)seed, batch)) return 1;
    for (long long i = 0; i < n; ++i)
        if (!m.sample(id_at((uint64_t)i, (uint64_t)seed, (int)bits))) return 1;
    if (rsv_count(m.h) + (int64_t)m.elems.size() != n) {
        std::printf("count %lld != %lld\n", (long long)rsv_count(m.h), n);
        return 1;
    }
    std::vector<int64_t> got;
    if (!m.result(&got)) return 1;
    std::sort(got.begin(), got.end());
    if (got != want) {
        std::printf("MISMATCH: %zu ids vs %zu expected\n", got.size(), want.size());
        return 1;
    }
    std::printf("ok n=%lld k=%lld candidates=%lld\n", n, k, (long long)m.candidates);
    return 0;
}
