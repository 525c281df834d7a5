// The block index of the prefix cache.  Host only: no HIP, no engine type, no device pointer — it names KV pages by number
// and counts their holders in the page_refs array it is given (tests/prefix_cache_model.cpp drives it stand-alone).
//
// A block is one full KV page: 64 prompt positions that a chunked-fill pass wrote.  Its identity is (parent block, its 64 token ids, the
// 16-byte key of the image if a pad lies in the block or before it).  The ids and the key are kept in the entry and compared on lookup:
// the hash only finds candidates.  A resident block IS its page, so a block is named by its page number and the root by -1.
//
// The index holds one reference on every cached page.  A page whose only holder is the index is evictable; a lease holds one more
// reference on every page of its chain, so nothing a lease names can go.  Whoever holds a block's page holds the pages of all its
// ancestors (a slot gets a chain whole, from a lease or by filling it), and a touch stamps a whole chain: a parent is never older than
// its child, and eviction — oldest stamp first, deepest block first among equally old — never orphans a resident block.
#pragma once

#include <cstdint>
#include <cstring>
#include <unordered_map>
#include <vector>

namespace prefix_cache {

constexpr int BLOCK = 64;                      // positions of a block = tokens of a KV page

// the pads of a prompt's image: positions [first, first + n); n == 0: no image; runs > 1: more than one image (not cached)
struct Pads { int first = 0, n = 0, runs = 0; };
inline Pads find_pads(const int32_t* ids, int len, int32_t image_token) {
    Pads p;
    for (int i = 0; i < len; ++i) {
        if (ids[i] != image_token) continue;
        if (i == 0 || ids[i - 1] != image_token) p.runs += 1;
        if (p.n++ == 0) p.first = i;
    }
    return p;
}

struct Info { int64_t lookups = 0, hit_tokens = 0, inserted = 0, evicted = 0; };

struct Lease {
    std::vector<int32_t> chain;                // the pages of positions [0, 64 * chain.size()), in order
    int32_t tail_page = -1;                    // >= 0: the block whose retained tower rows cover every image position behind the chain
    int hit_tokens = 0, needs_tower = 0;
};

class Index {
public:
    // refs: the holders of every page (the engine's page_refs); it outlives the index
    Index(std::vector<int32_t>* refs, int n_pages, int32_t image_token) : refs_(refs), image_token_(image_token), entries_(n_pages) {}

    // may a prompt use the cache at all: at most one image, and a key if it has one
    bool eligible(const int32_t* ids, int len, const uint8_t* key) const {
        const Pads p = find_pads(ids, len, image_token_);
        return p.runs <= 1 && (p.n == 0 || key != nullptr);
    }

    // Walks the chain of the prompt's full blocks.  hit = min(64 * matched, 64 * ((len - 1) / 64)): one position at least is always
    // computed.  needs_tower == 0: no image position at or behind `hit`, or a resident block retains the tower rows of all of them.
    // Returns the lease (> 0) that pins what the answer relies on, or 0 when it relies on nothing.  The caller has checked eligible().
    int lookup(const int32_t* ids, int len, const uint8_t* key, int* hit_tokens, int* needs_tower) {
        const Pads pads = find_pads(ids, len, image_token_);
        Lease l;
        int32_t parent = -1;
        const int cap = (len - 1) / BLOCK;
        for (int b = 0; b < cap; ++b) {
            const int32_t page = find(parent, ids + b * BLOCK, block_key(pads, b, key));
            if (page < 0) break;
            l.chain.push_back(page);
            parent = page;
        }
        l.hit_tokens = (int)l.chain.size() * BLOCK;
        const int last_pad = pads.first + pads.n - 1;
        if (pads.n && last_pad >= l.hit_tokens) {
            l.needs_tower = 1;
            // every image position still to fill lies in the page behind the chain, and a child of the chain's end retains those rows
            if (last_pad < l.hit_tokens + BLOCK) {
                auto range = tails_.equal_range(hash_tail(parent, key));
                for (auto it = range.first; it != range.second; ++it) {
                    if (tail_fits(entries_[it->second], parent, key, pads, l.hit_tokens)) {
                        l.tail_page = it->second;
                        l.needs_tower = 0;
                        break;
                    }
                }
            }
        }
        info_.lookups += 1;
        info_.hit_tokens += l.hit_tokens;
        *hit_tokens = l.hit_tokens;
        *needs_tower = l.needs_tower;
        if (l.chain.empty() && l.tail_page < 0) return 0;
        const uint64_t now = ++clock_;
        for (int32_t p : l.chain) { (*refs_)[p] += 1; entries_[p].stamp = now; }
        if (l.tail_page >= 0) {
            (*refs_)[l.tail_page] += 1;
            for (int32_t p = l.tail_page; p >= 0; p = entries_[p].parent) entries_[p].stamp = now;
        }
        const int id = ++lease_seq_;
        leases_.emplace(id, std::move(l));
        return id;
    }
    const Lease* lease(int id) const {
        auto it = leases_.find(id);
        return it == leases_.end() ? nullptr : &it->second;
    }
    // the lease lets go of its pages (they stay cached: the index holds them)
    bool release(int id) {
        auto it = leases_.find(id);
        if (it == leases_.end()) return false;
        for (int32_t p : it->second.chain) (*refs_)[p] -= 1;
        if (it->second.tail_page >= 0) (*refs_)[it->second.tail_page] -= 1;
        leases_.erase(it);
        return true;
    }
    int leases() const { return (int)leases_.size(); }
    void release_all() {
        while (!leases_.empty()) release(leases_.begin()->first);
    }
    // was the lease taken for this prompt: its chain is what the prompt's blocks find now (its pages cannot have gone meanwhile)
    bool matches(int id, const int32_t* ids, int len, const uint8_t* key) const {
        const Lease* l = lease(id);
        if (!l || (int)l->chain.size() > (len - 1) / BLOCK || (l->tail_page >= 0 && !key)) return false;
        const Pads pads = find_pads(ids, len, image_token_);
        int32_t parent = -1;
        for (size_t b = 0; b < l->chain.size(); ++b) {
            if (find(parent, ids + b * BLOCK, block_key(pads, (int)b, key)) != l->chain[b]) return false;
            parent = l->chain[b];
        }
        if (l->tail_page < 0) return l->needs_tower || !pads.n || pads.first + pads.n <= l->hit_tokens;
        return pads.n && pads.first + pads.n <= l->hit_tokens + BLOCK && tail_fits(entries_[l->tail_page], parent, key, pads, l->hit_tokens);
    }

    // Block `block` of the prompt, just written into `page` behind `parent` (-1: the root): the index takes a reference.  False: an equal
    // block is resident already (the caller's page stays its own, and it inserts nothing behind it), or the page is one.
    bool insert(int32_t parent, const int32_t* ids, int len, int block, const uint8_t* key, int32_t page) {
        const Pads pads = find_pads(ids, len, image_token_);
        const uint8_t* bk = block_key(pads, block, key);
        if (entries_[page].on || find(parent, ids + block * BLOCK, bk) >= 0) return false;
        Entry& n = entries_[page];
        n = Entry{};
        n.on = true;
        n.parent = parent;
        n.depth = block;
        std::memcpy(n.ids, ids + block * BLOCK, sizeof(n.ids));
        n.keyed = bk != nullptr;
        if (bk) std::memcpy(n.key, bk, 16);
        const int lo = block * BLOCK, last_pad = pads.first + pads.n - 1;
        if (pads.n && last_pad >= lo && last_pad < lo + BLOCK) {          // the image ends in this page: its rows here are retained
            n.tail = true;
            n.pad0 = pads.first > lo ? pads.first - lo : 0;
            n.row0 = pads.first > lo ? 0 : lo - pads.first;
            n.pad_n = pads.n - n.row0;
            tails_.emplace(hash_tail(parent, n.key), page);
        }
        table_.emplace(hash_block(parent, n.ids, bk), page);
        (*refs_)[page] += 1;
        const uint64_t now = ++clock_;
        for (int32_t p = page; p >= 0; p = entries_[p].parent) entries_[p].stamp = now;
        info_.inserted += 1;
        resident_ += 1;
        return true;
    }
    bool resident(int32_t page) const { return page >= 0 && page < (int32_t)entries_.size() && entries_[page].on; }
    // of a resident block that retains tower rows: offsets [pad0, pad0 + pad_n) of its page
    bool tail_rows(int32_t page, int* pad0, int* pad_n) const {
        if (!resident(page) || !entries_[page].tail) return false;
        *pad0 = entries_[page].pad0;
        *pad_n = entries_[page].pad_n;
        return true;
    }

    int resident_pages() const { return resident_; }
    int evictable_pages() const {
        int n = 0;
        for (size_t p = 0; p < entries_.size(); ++p) n += entries_[p].on && (*refs_)[p] == 1;
        return n;
    }
    // The least recently used evictable block, the deepest among equally old, leaves the index; its page (holders now 0) is the caller's
    // to put into the free list.  -1: nothing is evictable.
    int32_t evict_one() {
        int32_t best = -1;
        for (int32_t p = 0; p < (int32_t)entries_.size(); ++p) {
            const Entry& c = entries_[p];
            if (!c.on || (*refs_)[p] != 1) continue;
            if (best < 0 || c.stamp < entries_[best].stamp || (c.stamp == entries_[best].stamp && c.depth > entries_[best].depth)) best = p;
        }
        if (best < 0) return -1;
        drop(best);
        info_.evicted += 1;
        return best;
    }
    // Every block leaves (leases included); pages whose holders fall to 0 are appended to *freed
    void clear(std::vector<int32_t>* freed) {
        release_all();
        for (int32_t p = 0; p < (int32_t)entries_.size(); ++p)
            if (entries_[p].on) {
                drop(p);
                if ((*refs_)[p] == 0) freed->push_back(p);
            }
    }
    const Info& info() const { return info_; }

private:
    struct Entry {
        bool on = false, keyed = false, tail = false;
        int32_t parent = -1;
        int depth = 0, pad0 = 0, pad_n = 0, row0 = 0;      // tail: the pads at offsets [pad0, pad0 + pad_n) are rows [row0, row0 + pad_n) of the image, its last ones
        uint64_t stamp = 0;
        uint8_t key[16] = {0};
        int32_t ids[BLOCK] = {0};
    };
    // the key a block carries: the image's, if a pad lies in the block or before it
    static const uint8_t* block_key(const Pads& pads, int block, const uint8_t* key) { return pads.n && pads.first < (block + 1) * BLOCK ? key : nullptr; }
    static uint64_t mix(uint64_t h, const void* p, size_t n) {          // FNV-1a: finds candidates, never decides
        const uint8_t* b = static_cast<const uint8_t*>(p);
        for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 1099511628211ull;
        return h;
    }
    static uint64_t hash_block(int32_t parent, const int32_t* ids, const uint8_t* key) {
        uint64_t h = mix(14695981039346656037ull, &parent, 4);
        h = mix(h, ids, BLOCK * 4);
        return key ? mix(h, key, 16) : h;
    }
    static uint64_t hash_tail(int32_t parent, const uint8_t* key) { return mix(mix(14695981039346656037ull, &parent, 4), key, 16); }
    // does the block retain the image rows of every pad at or behind `hit` (all of which lie in the page behind it)
    static bool tail_fits(const Entry& t, int32_t parent, const uint8_t* key, const Pads& pads, int hit) {
        const int pad0 = pads.first > hit ? pads.first - hit : 0, row0 = pads.first > hit ? 0 : hit - pads.first;
        return t.on && t.tail && t.parent == parent && !std::memcmp(t.key, key, 16) && t.pad0 == pad0 && t.row0 == row0 && t.pad_n == pads.n - row0;
    }
    int32_t find(int32_t parent, const int32_t* ids, const uint8_t* key) const {
        auto range = table_.equal_range(hash_block(parent, ids, key));
        for (auto it = range.first; it != range.second; ++it) {
            const Entry& c = entries_[it->second];
            if (c.parent == parent && c.keyed == (key != nullptr) && !std::memcmp(c.ids, ids, sizeof(c.ids)) && (!key || !std::memcmp(c.key, key, 16)))
                return it->second;
        }
        return -1;
    }
    template <typename Map>
    static void erase_value(Map& m, uint64_t h, int32_t page) {
        auto range = m.equal_range(h);
        for (auto it = range.first; it != range.second; ++it)
            if (it->second == page) { m.erase(it); return; }
    }
    void drop(int32_t page) {
        Entry& c = entries_[page];
        erase_value(table_, hash_block(c.parent, c.ids, c.keyed ? c.key : nullptr), page);
        if (c.tail) erase_value(tails_, hash_tail(c.parent, c.key), page);
        c.on = false;
        (*refs_)[page] -= 1;
        resident_ -= 1;
    }

    std::vector<int32_t>* refs_;
    int32_t image_token_;
    std::vector<Entry> entries_;               // by page number
    std::unordered_multimap<uint64_t, int32_t> table_, tails_;
    std::unordered_map<int, Lease> leases_;
    Info info_;
    uint64_t clock_ = 0;
    int lease_seq_ = 0, resident_ = 0;
};

}  // namespace prefix_cache
