// A stand-alone run of the host trie (csrc/trie_host.cpp) for a sanitizer build on the CPU (tests/test_trie_capi.py): build, info, walks inside, at the
// ends of and outside the trie, the bad inputs, free.  Prints "ok" and returns 0 when every answer is the expected one.
#include <cstdio>
#include <cstring>
#include <random>
#include <set>
#include <vector>

#include "../biogpt.cpp_amd/csrc/host_common.h"

#define CHECK(cond)                                                   \
    do {                                                              \
        if (!(cond)) {                                                \
            std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond);   \
            return 1;                                                 \
        }                                                             \
    } while (0)

static std::vector<int32_t> allowed(const biogpt_hip_trie *t, const std::vector<int32_t> &gen, int32_t eos, int32_t cap = -1) {
    const int32_t n = biogpt_hip_trie_allowed_host(t, gen.data(), (int32_t)gen.size(), eos, nullptr, 0);
    if (n < 0) return {-1};
    std::vector<int32_t> out((size_t)(cap < 0 ? n : cap));      // exactly as large as the call may write
    const int32_t m = biogpt_hip_trie_allowed_host(t, gen.data(), (int32_t)gen.size(), eos, out.data(), (int32_t)out.size());
    if (m != n) return {-2};
    return out;
}

int main() {
    using V = std::vector<int32_t>;
    {   // duplicates, a prefix entry, tokens 0 and n_vocab - 1
        const V seqs{1, 2, 3, 1, 2, 1, 2, 3, 0, 1, 5, 99}, lens{3, 2, 3, 1, 3};
        biogpt_hip_trie *t = biogpt_hip_trie_build(seqs.data(), lens.data(), 5, 100);
        CHECK(t);
        int64_t info[5];
        CHECK(biogpt_hip_trie_info(t, info) == 0);
        CHECK(info[0] == 4 && info[1] == 7 && info[2] == 6 && info[3] == 3 && info[4] == 2);
        CHECK((allowed(t, {}, 50) == V{0, 1}));
        CHECK((allowed(t, {1}, 50) == V{2, 5}));
        CHECK((allowed(t, {1, 2}, 50) == V{3, 50}));
        CHECK((allowed(t, {1, 2}, 2) == V{2, 3}));
        CHECK((allowed(t, {1, 2, 3}, 50) == V{50}));
        CHECK((allowed(t, {1, 5}, 98) == V{99}));
        CHECK((allowed(t, {7}, 50) == V{50}));            // leaves the trie at the first token
        CHECK((allowed(t, {1, 2, 4}, 50) == V{50}));      // ... at the last
        CHECK((allowed(t, {1, 2, 3, 3}, 50) == V{50}));   // ... behind a leaf
        CHECK((allowed(t, {1, 2}, 50, 1) == V{3}));       // a short buffer takes the first ids and the size comes back
        CHECK(biogpt_hip_trie_allowed_host(t, nullptr, 1, 50, nullptr, 0) == -1 && std::strstr(bg::last_error(), "gen"));
        CHECK(biogpt_hip_trie_allowed_host(t, nullptr, -1, 50, nullptr, 0) == -1 && std::strstr(bg::last_error(), "n_gen"));
        CHECK(biogpt_hip_trie_allowed_host(t, nullptr, 0, 100, nullptr, 0) == -1 && std::strstr(bg::last_error(), "eos_id"));
        CHECK(biogpt_hip_trie_allowed_host(t, nullptr, 0, -1, nullptr, 0) == -1 && std::strstr(bg::last_error(), "eos_id"));
        CHECK(biogpt_hip_trie_allowed_host(t, nullptr, 0, 50, nullptr, 4) == -1 && std::strstr(bg::last_error(), "out_ids"));
        CHECK(biogpt_hip_trie_allowed_host(nullptr, nullptr, 0, 50, nullptr, 0) == -1 && std::strstr(bg::last_error(), "trie"));
        CHECK(biogpt_hip_trie_info(nullptr, info) == -1 && biogpt_hip_trie_info(t, nullptr) == -1);
        biogpt_hip_trie_free(t);
        biogpt_hip_trie_free(nullptr);
    }
    {   // the bad inputs of build
        const V seqs{1, 2, 3}, one{3}, zero{0}, two{1, 2};
        const V neg{1, -1, 3}, big{1, 100, 3};
        CHECK(!biogpt_hip_trie_build(seqs.data(), one.data(), 0, 100) && std::strstr(bg::last_error(), "n_seqs"));
        CHECK(!biogpt_hip_trie_build(seqs.data(), zero.data(), 1, 100) && std::strstr(bg::last_error(), "lens"));
        CHECK(!biogpt_hip_trie_build(neg.data(), one.data(), 1, 100) && std::strstr(bg::last_error(), "seqs"));
        CHECK(!biogpt_hip_trie_build(big.data(), one.data(), 1, 100) && std::strstr(bg::last_error(), "seqs"));
        CHECK(!biogpt_hip_trie_build(nullptr, one.data(), 1, 100) && std::strstr(bg::last_error(), "seqs"));
        CHECK(!biogpt_hip_trie_build(seqs.data(), nullptr, 1, 100) && std::strstr(bg::last_error(), "lens"));
        CHECK(!biogpt_hip_trie_build(seqs.data(), one.data(), 1, 0) && std::strstr(bg::last_error(), "n_vocab"));
    }
    {   // random entries against a set of prefixes: fan-out 4097 at the root, depth up to 63
        const int32_t nv = 5000, eos = 4999;
        std::mt19937 rng(7);
        V seqs, lens;
        std::set<V> prefixes, entries;
        auto add = [&](const V &e) {
            seqs.insert(seqs.end(), e.begin(), e.end());
            lens.push_back((int32_t)e.size());
            entries.insert(e);
            for (size_t n = 0; n <= e.size(); n++) prefixes.insert(V(e.begin(), e.begin() + (long)n));
        };
        for (int32_t t = 0; t < 4097; t++) add(V{t});
        for (int i = 0; i < 300; i++) {
            V e((size_t)(1 + rng() % 63));
            for (auto &t : e) t = (int32_t)(rng() % 6);
            add(e);
        }
        biogpt_hip_trie *t = biogpt_hip_trie_build(seqs.data(), lens.data(), (int32_t)lens.size(), nv);
        CHECK(t);
        int64_t info[5];
        CHECK(biogpt_hip_trie_info(t, info) == 0);
        CHECK(info[0] == (int64_t)entries.size() && info[1] == (int64_t)prefixes.size() && info[2] == info[1] - 1 && info[4] == 4097);
        for (const V &p : prefixes) {
            V want;
            for (int32_t tk = 0; tk < 4097; tk++) {
                V q(p);
                q.push_back(tk);
                if (prefixes.count(q)) want.push_back(tk);
                if (p.size() > 0 && tk >= 6) break;      // (below the root only the tokens 0 .. 5 occur)
            }
            if (entries.count(p)) want.push_back(eos);
            CHECK(allowed(t, p, eos) == want);
        }
        biogpt_hip_trie_free(t);
    }
    std::puts("ok");
    return 0;
}
