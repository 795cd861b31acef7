// pkeys.h -- parameter value -> 64-bit key, exactly: equal keys only for equal values.
//
// ParamFlowChecker keeps one token bucket, throttle clock and thread count per argument value, in maps that
// compare values with equals() (param/slots/block/flow/param/ParameterMetric.java:88-104).  The device maps are
// keyed by a 64-bit word.  For int, long within +-2^59, float, byte, short, boolean and char that word holds the
// value (the pure key below); for Strings, longs outside +-2^59 and doubles it is a 60-bit hash, so two values
// can share it.  The dictionary here gives every hashed value that is in use an entry and a key no other entry
// owns: the pure key for the first owner, a stepped key for a value whose pure key is taken.  A value that
// collides with nothing keeps its pure key, so callers of the pure function and of the dictionary interoperate.
//
// Host C++ only (no HIP types).  The hash is a template parameter so that a test can inject a weak one.
//
// Lifetime: every entry carries `touched`, the epoch of its last intern.  sweep_begin() opens a new epoch and
// lists the unpinned entries not touched in the one before; the caller finds out which of those keys the device
// still holds; sweep_finish() drops the others, checking `touched` again (an intern may have hit a candidate in
// between).  Pinned entries (hot items of loaded rules) are never candidates.
#pragma once
#include <atomic>
#include <cctype>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <shared_mutex>
#include <string>
#include <unordered_map>
#include <vector>

namespace sg {
namespace pk {

constexpr uint64_t KEY_MASK = 0x0FFFFFFFFFFFFFFFULL;
constexpr uint64_t LONG_HASHED = 1ULL << 59;  // tag 3: set in the key of a long outside +-2^59
inline uint64_t tagged(uint64_t tag, uint64_t v) { return (tag << 60) | (v & KEY_MASK); }
inline uint64_t mix64(uint64_t x) {
    x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ULL;
    x ^= x >> 27; x *= 0x94d049bb133111ebULL;
    x ^= x >> 31; return x;
}
// the hash of the pure keys: FNV-1a over the text, mix64 over a double's bits
struct StdHash {
    static uint64_t text(const char* s) {
        uint64_t h = 1469598103934665603ULL;
        for (; *s; ++s) { h ^= (unsigned char)*s; h *= 1099511628211ULL; }
        return h;
    }
    static uint64_t bits(uint64_t u) { return mix64(u); }
};

inline bool blank(const char* s) {
    if (!s) return true;
    for (; *s; ++s)
        if (*s != ' ' && *s != '\t' && *s != '\n' && *s != '\r' && *s != '\f' && *s != '\v') return false;
    return true;
}
inline bool ieq(const char* a, const char* b) {
    for (; *a && *b; ++a, ++b) if (std::tolower((unsigned char)*a) != std::tolower((unsigned char)*b)) return false;
    return *a == *b;
}

// A value as ParamFlowRuleUtil.parseItemValue types it (ParamFlowRuleUtil.java:85-121): its pure key, and for
// the hashed kinds the bytes that decide equality (*canon if asked for, prefixed with the tag).
struct Typed {
    uint64_t pure = 0;
    uint32_t tag = 0;
    bool hashed = false;
};
template <class H>
inline void classify(const char* v, const char* t, Typed& o, std::string* canon = nullptr) {
    o.hashed = false;
    auto is = [&](const char* a, const char* b) { return t && (!std::strcmp(t, a) || !std::strcmp(t, b)); };
    auto text = [&]() {  // String, and every class the caller turned into text
        o.tag = 1;
        o.pure = tagged(1, H::text(v) & KEY_MASK);
        o.hashed = true;
        if (canon) { canon->assign(1, (char)1); canon->append(v); }
    };
    auto raw8 = [&](uint32_t tag, uint64_t u) {
        canon->assign(1, (char)tag);
        canon->append(reinterpret_cast<const char*>(&u), 8);
    };
    if (blank(t) || !std::strcmp(t, "java.lang.String") || !std::strcmp(t, "String")) return text();
    if (is("int", "java.lang.Integer")) { o.tag = 2; o.pure = tagged(2, (uint32_t)(int32_t)std::strtol(v, nullptr, 10)); return; }
    if (is("long", "java.lang.Long")) {
        const long long x = std::strtoll(v, nullptr, 10);
        o.tag = 3;
        if (x >= -(1LL << 59) && x < (1LL << 59)) { o.pure = tagged(3, (uint64_t)x); return; }
        o.pure = tagged(3, (H::text(v) & KEY_MASK) | LONG_HASHED);
        o.hashed = true;
        if (canon) raw8(3, (uint64_t)x);  // Long.equals: the parsed value
        return;
    }
    if (is("double", "java.lang.Double")) {
        const double d = std::strtod(v, nullptr);
        uint64_t u;
        std::memcpy(&u, &d, 8);
        o.tag = 4;
        o.pure = tagged(4, H::bits(u));
        o.hashed = true;
        // Double.equals compares doubleToLongBits: 0.0 != -0.0, and every NaN is the one canonical NaN
        if (canon) raw8(4, d != d ? 0x7ff8000000000000ULL : u);
        return;
    }
    if (is("float", "java.lang.Float")) {
        const float f = std::strtof(v, nullptr);
        uint32_t u;
        std::memcpy(&u, &f, 4);
        o.tag = 5; o.pure = tagged(5, u);
        return;
    }
    if (is("byte", "java.lang.Byte")) { o.tag = 6; o.pure = tagged(6, (uint8_t)(int8_t)std::strtol(v, nullptr, 10)); return; }
    if (is("short", "java.lang.Short")) { o.tag = 7; o.pure = tagged(7, (uint16_t)(int16_t)std::strtol(v, nullptr, 10)); return; }
    if (is("boolean", "java.lang.Boolean")) { o.tag = 8; o.pure = tagged(8, ieq(v, "true") ? 1 : 0); return; }
    if (!std::strcmp(t, "char")) { o.tag = 9; o.pure = tagged(9, (unsigned char)v[0]); return; }
    return text();
}
// the pure function (sg_param_key): NULL -> 0
template <class H = StdHash>
inline uint64_t pure_key(const char* v, const char* t) {
    if (!v) return 0;
    // the String case first and on its own: it is nearly every call, and the caller's loop is a few ns a key
    if (blank(t) || !std::strcmp(t, "java.lang.String") || !std::strcmp(t, "String")) return tagged(1, H::text(v) & KEY_MASK);
    Typed x;
    classify<H>(v, t, x);
    return x.pure;
}

struct Stats {
    uint64_t entries = 0, displaced = 0, pinned = 0;
};

template <class H = StdHash>
class Dict {
  public:
    // The value's key; a hashed kind gets (or keeps) an entry, touched now.  pin: the entry is pinned once more
    // (unpin() with the returned key undoes it).  *has_entry: the value is of a hashed kind.  NULL -> 0.
    uint64_t intern(const char* v, const char* t, bool pin = false, bool* has_entry = nullptr) {
        if (has_entry) *has_entry = false;
        if (!v) return 0;
        Typed x;
        thread_local std::string canon;  // (a hit allocates nothing once the buffer has grown)
        classify<H>(v, t, x, &canon);
        if (!x.hashed) return x.pure;
        if (has_entry) *has_entry = true;
        if (!pin) {
            std::shared_lock<std::shared_mutex> lk(mu_);
            auto it = by_value_.find(canon);
            if (it != by_value_.end()) {
                it->second->touched.store(epoch_, std::memory_order_relaxed);
                return it->second->key;
            }
        }
        std::unique_lock<std::shared_mutex> lk(mu_);
        auto it = by_value_.find(canon);
        if (it != by_value_.end()) {
            Entry& e = *it->second;
            e.touched.store(epoch_, std::memory_order_relaxed);
            if (pin && e.pins++ == 0) ++n_pinned_;
            return e.key;
        }
        std::unique_ptr<Entry> e(new Entry);
        e->key = free_key(x.pure, x.tag);
        e->pure = x.pure;
        e->pins = pin ? 1 : 0;
        e->touched.store(epoch_, std::memory_order_relaxed);
        const uint64_t k = e->key;
        if (pin) ++n_pinned_;
        if (k != x.pure) ++n_displaced_;
        auto ins = by_value_.emplace(canon, std::move(e));
        ins.first->second->value = &ins.first->first;
        by_key_[k] = ins.first->second.get();
        return k;
    }
    // The inverse: the canonical bytes (tag byte, then the text or the 8 raw bytes) of the entry that owns key.
    // False when no entry does, as for a pure key that was never interned.  Does not touch the entry.
    bool value_of(uint64_t key, std::string& canon) const {
        std::shared_lock<std::shared_mutex> lk(mu_);
        auto it = by_key_.find(key);
        if (it == by_key_.end()) return false;
        canon = *it->second->value;
        return true;
    }
    void unpin(uint64_t key) {
        std::unique_lock<std::shared_mutex> lk(mu_);
        auto it = by_key_.find(key);
        if (it == by_key_.end() || it->second->pins == 0) return;
        if (--it->second->pins == 0) --n_pinned_;
    }
    // Open epoch E + 1 and list the candidates of sweep E: the keys of the unpinned entries with touched < E.
    uint64_t sweep_begin(std::vector<uint64_t>& cand) {
        std::unique_lock<std::shared_mutex> lk(mu_);
        const uint64_t E = epoch_;
        epoch_ = E + 1;
        cand.clear();
        for (const auto& kv : by_key_)
            if (kv.second->pins == 0 && kv.second->touched.load(std::memory_order_relaxed) < E) cand.push_back(kv.first);
        return E;
    }
    // Drop the candidates whose bit in `held` (bit i of word i / 32 = cand[i]) is clear and that are still
    // unpinned and untouched since before E.  Returns how many were dropped.
    uint64_t sweep_finish(uint64_t E, const std::vector<uint64_t>& cand, const uint32_t* held) {
        std::unique_lock<std::shared_mutex> lk(mu_);
        uint64_t dropped = 0;
        for (size_t i = 0; i < cand.size(); ++i) {
            if (held && ((held[i >> 5] >> (i & 31)) & 1u)) continue;
            auto it = by_key_.find(cand[i]);
            if (it == by_key_.end()) continue;
            Entry* e = it->second;
            if (e->pins || e->touched.load(std::memory_order_relaxed) >= E) continue;
            if (e->key != e->pure) --n_displaced_;
            auto vit = by_value_.find(*e->value);
            by_key_.erase(it);
            by_value_.erase(vit);  // (frees e)
            ++dropped;
        }
        return dropped;
    }
    Stats stats() const {
        std::shared_lock<std::shared_mutex> lk(mu_);
        Stats s;
        s.entries = by_value_.size();
        s.displaced = n_displaced_;
        s.pinned = n_pinned_;
        return s;
    }
    uint64_t epoch() const {
        std::shared_lock<std::shared_mutex> lk(mu_);
        return epoch_;
    }

  private:
    struct Entry {
        uint64_t key = 0, pure = 0;
        uint32_t pins = 0;                    // written under the exclusive lock
        std::atomic<uint64_t> touched{0};     // a hit stores it under the shared lock
        const std::string* value = nullptr;   // its key in by_value_ (node addresses are stable)
    };
    // The first key from the pure key on that no entry owns.  A step keeps the tag nibble (so the key is never
    // 0 and never all-ones: tags are 1..9) and, for a hashed long, the bit that tells it from the longs in range.
    uint64_t free_key(uint64_t pure, uint32_t tag) const {
        const uint64_t keep = tag == 3 ? LONG_HASHED : 0;
        uint64_t c = pure;
        for (uint64_t n = 1; by_key_.count(c); ++n) {
            // mix64 is a bijection of 2^64 and by_key_ is finite; past 64 steps walk the 60-bit space in order
            c = n <= 64 ? tagged(tag, mix64(c + n * 0x9E3779B97F4A7C15ULL) | keep) : tagged(tag, (c + 1) | keep);
        }
        return c;
    }

    mutable std::shared_mutex mu_;
    uint64_t epoch_ = 0;
    uint64_t n_displaced_ = 0, n_pinned_ = 0;
    std::unordered_map<std::string, std::unique_ptr<Entry>> by_value_;
    std::unordered_map<uint64_t, Entry*> by_key_;
};

} // namespace pk
} // namespace sg
