// Drives the block index of the prefix cache (csrc/prefix_cache.h) without an engine: a vector of holder counts stands for page_refs and a
// small "slot" stands for a sequence that fills a prompt and inserts its full pages.  Prints "N checks" and exits 0 when every one held.
#include <cstdio>
#include <cstdlib>
#include <numeric>

#include "prefix_cache.h"

using prefix_cache::Index;

static long n_checks = 0;
#define CHECK(x)                                                                   \
    do {                                                                           \
        ++n_checks;                                                                \
        if (!(x)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); std::exit(1); } \
    } while (0)

constexpr int32_t IMG = 9999;
constexpr int N_PAGES = 48;

struct Pool {
    std::vector<int32_t> refs = std::vector<int32_t>(N_PAGES, 0), free_list;
    Index idx{&refs, N_PAGES, IMG};
    Pool() { for (int p = N_PAGES - 1; p >= 0; --p) free_list.push_back(p); }
    int32_t take() {
        if (free_list.empty()) {
            const int32_t p = idx.evict_one();
            CHECK(p >= 0 && refs[p] == 0);
            return p;
        }
        const int32_t p = free_list.back();
        free_list.pop_back();
        return p;
    }
    // a sequence fills the prompt behind `lease` (0: cold), inserts its full pages and is released; returns its pages
    std::vector<int32_t> fill(const std::vector<int32_t>& ids, const uint8_t* key, int lease = 0, bool release = true) {
        std::vector<int32_t> pages;
        int32_t parent = -1;
        if (lease) {
            CHECK(idx.matches(lease, ids.data(), (int)ids.size(), key));
            for (int32_t p : idx.lease(lease)->chain) { pages.push_back(p); refs[p] += 1; parent = p; }
        }
        const int n = ((int)ids.size() + 63) / 64;
        bool on = idx.eligible(ids.data(), (int)ids.size(), key);
        for (int k = (int)pages.size(); k < n; ++k) {
            pages.push_back(take());
            refs[pages.back()] = 1;
            if (on && (k + 1) * 64 <= (int)ids.size()) {
                if (idx.insert(parent, ids.data(), (int)ids.size(), k, key, pages.back())) parent = pages.back();
                else on = false;
            }
        }
        if (lease) CHECK(idx.release(lease));
        if (release) drop(pages);
        return pages;
    }
    void drop(const std::vector<int32_t>& pages) {
        for (int32_t p : pages)
            if (--refs[p] == 0) free_list.push_back(p);
    }
};

static std::vector<int32_t> text(int len, int seed) {
    std::vector<int32_t> v(len);
    for (int i = 0; i < len; ++i) v[i] = (int32_t)((1103515245u * (unsigned)(i + 977 * seed) + 12345u) >> 8) % 5000;
    return v;
}
static std::vector<int32_t> with_image(std::vector<int32_t> v, int first, int n) {
    for (int i = 0; i < n; ++i) v[first + i] = IMG;
    return v;
}

int main() {
    uint8_t key_a[16], key_b[16];
    for (int i = 0; i < 16; ++i) { key_a[i] = (uint8_t)(i + 1); key_b[i] = (uint8_t)(31 * i + 7); }
    int hit = 0, tower = 0;

    // ---- chain match, and divergence at every offset of every page
    {
        Pool P;
        const auto a = text(300, 1);
        P.fill(a, nullptr);
        CHECK(P.idx.resident_pages() == 4 && P.idx.evictable_pages() == 4);          // 300 / 64 full pages: the ragged fifth is not cached
        for (int d = 0; d < 300; ++d) {
            auto b = a;
            b[d] += 1;
            const int lease = P.idx.lookup(b.data(), (int)b.size(), nullptr, &hit, &tower);
            CHECK(hit == 64 * std::min(d / 64, 4) && tower == 0);
            CHECK((lease != 0) == (hit > 0));
            if (lease) {
                CHECK((int)P.idx.lease(lease)->chain.size() == hit / 64 && P.idx.evictable_pages() == 4 - hit / 64);
                CHECK(P.idx.matches(lease, b.data(), (int)b.size(), nullptr) && !P.idx.matches(lease, text(300, 2).data(), 300, nullptr));
                CHECK(P.idx.release(lease) && !P.idx.release(lease));
            }
            CHECK(P.idx.evictable_pages() == 4);
        }
    }
    // ---- the (len - 1) / 64 cap: one position at least is computed
    {
        Pool P;
        const auto a = text(256, 3);
        P.fill(a, nullptr);
        CHECK(P.idx.resident_pages() == 4);
        for (int len = 1; len <= 256; ++len) {
            const int lease = P.idx.lookup(a.data(), len, nullptr, &hit, &tower);
            CHECK(hit == 64 * ((len - 1) / 64));
            if (lease) P.idx.release(lease);
        }
        // a repeat of the 256-token prompt fills its last page itself and finds the block resident: the page stays its own
        const int lease = P.idx.lookup(a.data(), 256, nullptr, &hit, &tower);
        CHECK(hit == 192);
        const long inserted = P.idx.info().inserted;
        P.fill(a, nullptr, lease);
        CHECK(P.idx.info().inserted == inserted && P.idx.resident_pages() == 4 && P.idx.leases() == 0);
    }
    // ---- the image key: in the pad block and in every block after it, not before it
    {
        Pool P;
        const auto a = with_image(text(400, 4), 70, 8);          // pads at 70 .. 77: block 1
        P.fill(a, key_a);
        CHECK(P.idx.resident_pages() == 6);
        int lease = P.idx.lookup(a.data(), 400, key_a, &hit, &tower);
        CHECK(hit == 384 && tower == 0);
        P.idx.release(lease);
        lease = P.idx.lookup(a.data(), 400, key_b, &hit, &tower);          // other pixels: block 0 has no pad yet and matches, block 1 does not
        CHECK(hit == 64 && tower == 1);
        P.idx.release(lease);
        CHECK(!P.idx.eligible(a.data(), 400, nullptr));                       // an image and no key: bypass
        CHECK(!P.idx.eligible(with_image(a, 200, 4).data(), 400, key_a));     // two images: bypass
        lease = P.idx.lookup(a.data(), 400, key_b, &hit, &tower);
        P.fill(a, key_b, lease);                                              // the same ids under the other key: its own blocks from block 1 on
        CHECK(P.idx.resident_pages() == 11);
        lease = P.idx.lookup(a.data(), 400, key_b, &hit, &tower);
        CHECK(hit == 384 && tower == 0);
        P.idx.release(lease);
        // a text prompt with the ids of block 0 shares block 0 and nothing else
        auto t = text(400, 4);
        lease = P.idx.lookup(t.data(), 400, nullptr, &hit, &tower);
        CHECK(hit == 64);
        P.idx.release(lease);
    }
    // ---- tail rows: the image ends in the page behind the hit and a resident child of the chain's end retains its rows there
    {
        Pool P;
        const auto a = with_image(text(233, 5), 60, 16);         // pads at 60 .. 75
        const auto pages = P.fill(a, key_a);
        auto b = a;
        for (int i = 100; i < 233; ++i) b[i] += 1;                // diverges at 100: block 1 differs, block 0 matches
        int lease = P.idx.lookup(b.data(), 233, key_a, &hit, &tower);
        CHECK(hit == 64 && tower == 0 && P.idx.lease(lease)->tail_page == pages[1]);
        int pad0 = -1, pad_n = -1;
        CHECK(P.idx.tail_rows(pages[1], &pad0, &pad_n) && pad0 == 0 && pad_n == 12);
        CHECK(!P.idx.tail_rows(pages[0], &pad0, &pad_n));
        CHECK(P.refs[pages[0]] == 2 && P.refs[pages[1]] == 2 && P.refs[pages[2]] == 1);
        P.idx.release(lease);
        lease = P.idx.lookup(b.data(), 233, key_b, &hit, &tower);          // other pixels: block 0 holds pads, so not even it matches
        CHECK(lease == 0 && hit == 0 && tower == 1);
        auto c = a;
        for (int i = 72; i < 76; ++i) c[i] = 17;                    // the image ends earlier: other pads, the rows do not fit
        lease = P.idx.lookup(c.data(), 233, key_a, &hit, &tower);
        CHECK(hit == 64 && tower == 1);
        P.idx.release(lease);
        // an image that runs beyond the page behind the hit needs its tower
        const auto d = with_image(text(400, 6), 60, 100);
        P.fill(d, key_b);
        auto d2 = d;
        d2[300] += 1;
        lease = P.idx.lookup(d2.data(), 400, key_b, &hit, &tower);
        CHECK(hit == 256 && tower == 0);                           // every pad lies before the hit
        P.idx.release(lease);
        d2 = d;
        d2[170] += 1;
        lease = P.idx.lookup(d2.data(), 400, key_b, &hit, &tower);
        CHECK(hit == 128 && tower == 0);                           // the pads end at 159, in the page behind the hit, whose block is resident
        P.idx.release(lease);
        d2 = d;
        d2[5] += 1;
        lease = P.idx.lookup(d2.data(), 400, key_b, &hit, &tower);
        CHECK(lease == 0 && hit == 0 && tower == 1);               // pads in pages 0, 1 and 2: more than the page behind the hit
    }
    // ---- eviction: least recently used first, deepest first among equally old; a lease holds its chain
    {
        Pool P;
        const auto a = text(200, 7), b = text(200, 8), c = text(200, 9);
        const auto pa = P.fill(a, nullptr), pb = P.fill(b, nullptr), pc = P.fill(c, nullptr);
        CHECK(P.idx.resident_pages() == 9 && P.idx.evictable_pages() == 9);
        int lease = P.idx.lookup(a.data(), 200, nullptr, &hit, &tower);       // touches a's whole chain: b is the oldest now
        CHECK(hit == 192);
        P.idx.release(lease);
        CHECK(P.idx.evict_one() == pb[2] && P.idx.evict_one() == pb[1] && P.idx.evict_one() == pb[0]);
        CHECK(P.idx.evict_one() == pc[2]);
        lease = P.idx.lookup(a.data(), 130, nullptr, &hit, &tower);           // pins a's blocks 0 and 1 and makes them younger than block 2
        CHECK(hit == 128 && P.idx.evictable_pages() == 3);
        CHECK(P.idx.evict_one() == pc[1] && P.idx.evict_one() == pc[0] && P.idx.evict_one() == pa[2]);
        CHECK(P.idx.evict_one() == -1 && P.idx.evictable_pages() == 0 && P.idx.resident_pages() == 2);
        CHECK(P.idx.release(lease) && P.idx.evictable_pages() == 2);
        CHECK(P.idx.evict_one() == pa[1] && P.idx.evict_one() == pa[0] && P.idx.evict_one() == -1);
        CHECK(P.idx.info().evicted == 9 && P.idx.resident_pages() == 0);
        lease = P.idx.lookup(a.data(), 200, nullptr, &hit, &tower);
        CHECK(lease == 0 && hit == 0);
    }
    // ---- a pool under pressure: a live sequence's pages never go, and every count returns to zero
    {
        Pool P;
        const auto live = P.fill(text(640, 10), nullptr, 0, false);          // 10 pages held by a live sequence, all full and cached
        for (int s = 11; s < 40; ++s) {
            P.fill(text(640, s), nullptr);                                     // 38 pages left for 10-page sequences: older ones must go
            for (int32_t p : live) CHECK(P.refs[p] == 2 && P.idx.resident(p));
            CHECK((int)P.free_list.size() + P.idx.resident_pages() == N_PAGES);
        }
        CHECK(P.idx.info().evicted > 0);
        P.drop(live);
        std::vector<int32_t> freed;
        P.idx.clear(&freed);
        CHECK(P.idx.resident_pages() == 0 && P.idx.leases() == 0);
        CHECK((int)(P.free_list.size() + freed.size()) == N_PAGES);
        CHECK(std::accumulate(P.refs.begin(), P.refs.end(), 0) == 0);
    }
    std::printf("%ld checks\n", n_checks);
    return 0;
}
