// Every decision of the content-ID set (kcdc_dedup.hip), as functions the device kernels and the
// stand-alone host program tools/dedup_host.cpp both run: the home slot, the fingerprint, the probe
// step and its wrap-around, the key compare at any alignment, the refusal rule, the sizes behind
// kcdc_dedup_bytes, and the four per-key steps (probe, outcome, commit, lookup) over a slot-word
// access policy: agent-scope atomics on the device, plain words in the sequential host program.
//
// A slot word is 64 bits: all ones when empty, else fingerprint (31 bits) << 32 | reference.  A
// reference with the top bit set is an index into the IDs of the running call; one without is an
// index into the set's key store.  Equal keys have equal fingerprints, so among the words of one key
// the smaller word is the smaller reference: a stored key beats every in-call one, and a lower
// index of the call a higher one.
#pragma once

#include <cstdint>

#include "kcdc_internal.h"  // KCDC_HD

namespace kcdc {
namespace dedupfmt {

constexpr uint32_t kMinIdLen = 16, kMaxIdLen = 32;  // every kcdc_hash_size
constexpr uint64_t kMaxKeys = 1ull << 31;
constexpr uint64_t kMinSlots = 16;
constexpr uint64_t kEmpty = ~0ull;
constexpr uint32_t kInCall = 0x80000000u;
constexpr uint32_t kKnown = 0xFFFFFFFFu;  // KCDC_DEDUP_KNOWN
constexpr int32_t kEnospc = -28;
// u64 words of a set.  Tickets: zeroed by a memset at the head of every call, one word per persistent
// kernel of the call.  Scalars: [0] keys stored.
constexpr uint32_t kTickets = 8, kTicketProbe = 0, kTicketOutcome = 1, kTicketCommit = 2;
constexpr uint32_t kScalars = 8, kStored = 0;
constexpr uint32_t kScanTile = 4096;  // keys per workgroup of the prefix sum

KCDC_HD inline bool valid_shape(uint32_t id_len, uint64_t max_keys) {
    return id_len >= kMinIdLen && id_len <= kMaxIdLen && max_keys >= 1 && max_keys <= kMaxKeys;
}

// The refusal rule: a call of n IDs is taken only if all of them could be new.
KCDC_HD inline bool refused(uint64_t stored, uint64_t n, uint64_t max_keys) { return stored + n > max_keys; }

// ---- sizes
// At least two slots per key the set can hold, a power of two: the load factor stays at or below 1/2
// and a probe always ends at an empty slot.
KCDC_HD inline uint64_t slot_count(uint64_t max_keys) {
    uint64_t s = kMinSlots;
    while (s < 2u * max_keys) s <<= 1;
    return s;
}
// A stored key: id_len hash bytes, the prefix byte, padded to a multiple of 4.
KCDC_HD inline uint32_t key_stride(uint32_t id_len) { return (id_len + 1u + 3u) & ~3u; }
KCDC_HD inline uint64_t scan_tiles(uint64_t max_keys) { return (max_keys + kScanTile - 1u) / kScanTile; }

struct Layout {  // offsets from the set's one allocation
    uint64_t tickets, scal, slots, store, slot_of, pos, tile_sums, total;
};
inline Layout layout(uint32_t id_len, uint64_t max_keys) {
    Layout l{};
    uint64_t at = 0;
    auto take = [&](uint64_t bytes) {
        const uint64_t o = at;
        at = (at + bytes + 255u) / 256u * 256u;
        return o;
    };
    l.tickets = take(kTickets * 8u);  // at the allocation's start, 64 bytes: the per-call memset
    l.scal = take(kScalars * 8u);
    l.slots = take(slot_count(max_keys) * 8u);
    l.store = take(max_keys * key_stride(id_len));
    l.slot_of = take(max_keys * 4u);                    // the slot each ID of a call ended its probe at
    l.pos = take((max_keys + 1u) * 4u);                 // keep flags, then their exclusive prefix sums
    l.tile_sums = take((scan_tiles(max_keys) + 1u) * 4u);
    l.total = at;
    return l;
}

// ---- keys
KCDC_HD inline uint32_t load32_any(const uint8_t* p) {
    if ((reinterpret_cast<uintptr_t>(p) & 3u) == 0) return *reinterpret_cast<const uint32_t*>(p);
    return uint32_t(p[0]) | uint32_t(p[1]) << 8 | uint32_t(p[2]) << 16 | uint32_t(p[3]) << 24;
}
KCDC_HD inline uint64_t load64_any(const uint8_t* p) { return load32_any(p) | uint64_t(load32_any(p + 4)) << 32; }

KCDC_HD inline uint64_t mix64(uint64_t x) {  // the 64-bit finalizer of MurmurHash3
    x ^= x >> 33;
    x *= 0xff51afd7ed558ccdull;
    x ^= x >> 33;
    x *= 0xc4ceb9fe1a85ec53ull;
    x ^= x >> 33;
    return x;
}
// Content IDs are hash outputs: the first 16 bytes and the prefix decide the slot.  IDs that agree
// in them share home and fingerprint and are told apart by the full compare.
KCDC_HD inline uint64_t key_hash(uint8_t prefix, const uint8_t* id) {
    return mix64(load64_any(id) ^ mix64(load64_any(id + 8) + (uint64_t(prefix) + 1u) * 0x9e3779b97f4a7c15ull));
}
KCDC_HD inline uint64_t home_slot(uint64_t h, uint64_t nslots) { return h & (nslots - 1u); }
KCDC_HD inline uint32_t fingerprint(uint64_t h) { return static_cast<uint32_t>(h >> 33); }  // 31 bits
KCDC_HD inline uint64_t next_slot(uint64_t s, uint64_t nslots) { return (s + 1u) & (nslots - 1u); }

KCDC_HD inline uint64_t slot_word(uint32_t fp, uint32_t ref) { return uint64_t(fp) << 32 | ref; }
KCDC_HD inline uint32_t word_fp(uint64_t w) { return static_cast<uint32_t>(w >> 32); }
KCDC_HD inline uint32_t word_ref(uint64_t w) { return static_cast<uint32_t>(w); }

// id_len bytes at a against id_len bytes at b, either at any alignment; reads no other byte.
KCDC_HD inline bool key_equal(const uint8_t* a, const uint8_t* b, uint32_t id_len) {
    const bool words = ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 3u) == 0;
    uint32_t i = 0, diff = 0;
    if (words)
        for (; i + 4u <= id_len; i += 4u)
            diff |= *reinterpret_cast<const uint32_t*>(a + i) ^ *reinterpret_cast<const uint32_t*>(b + i);
    for (; i < id_len; i++) diff |= uint32_t(a[i] ^ b[i]);
    return diff == 0;
}

// An array of keys: the caller's IDs under one prefix, or a key store, whose keys carry their own
// prefix in the byte after the ID.
struct Keys {
    const uint8_t* ids;
    uint64_t stride;
    uint32_t id_len;
    uint8_t prefix, stored;
};
KCDC_HD inline const uint8_t* key_id(const Keys& k, uint64_t i) { return k.ids + i * k.stride; }
KCDC_HD inline uint8_t key_prefix(const Keys& k, uint64_t i) { return k.stored ? key_id(k, i)[k.id_len] : k.prefix; }

struct Table {
    uint64_t* slots;
    uint64_t nslots;
    uint8_t* store;  // max_keys keys, key_stride apart
    uint32_t id_len;
};
KCDC_HD inline Keys store_keys(const Table& t) { return Keys{t.store, key_stride(t.id_len), t.id_len, 0, 1}; }

// Does the key a slot word refers to equal key i of the call?
KCDC_HD inline bool word_matches(const Table& t, const Keys& call, uint64_t w, uint32_t i, uint32_t fp) {
    if (word_fp(w) != fp) return false;
    const uint32_t ref = word_ref(w);
    const Keys other = ref & kInCall ? call : store_keys(t);
    const uint64_t j = ref & ~kInCall;
    return key_prefix(other, j) == key_prefix(call, i) && key_equal(key_id(other, j), key_id(call, i), t.id_len);
}

// ---- the per-key steps.  A: load / cas / min / store on a slot word.
// Probe for key i of the call and leave a reference to it, or to an equal key that goes before it,
// in the slot returned.  Never waits: every step either ends the probe or moves to the next slot,
// and an empty slot exists because the call was not refused.
template <class A>
KCDC_HD inline uint64_t probe_claim(const Table& t, const Keys& call, uint32_t i) {
    const uint64_t h = key_hash(key_prefix(call, i), key_id(call, i));
    const uint32_t fp = fingerprint(h);
    const uint64_t mine = slot_word(fp, kInCall | i);
    uint64_t s = home_slot(h, t.nslots);
    for (;;) {
        uint64_t w = A::load(t.slots + s);
        if (w == kEmpty) {
            w = A::cas(t.slots + s, kEmpty, mine);
            if (w == kEmpty) return s;
        }
        if (word_matches(t, call, w, i, fp)) {
            if (mine < w) A::min(t.slots + s, mine);
            return s;
        }
        s = next_slot(s, t.nslots);
    }
}

// After every probe of the call has ended: the lowest index of the call with key i's key, or kKnown.
template <class A>
KCDC_HD inline uint32_t outcome_first(const Table& t, uint64_t slot) {
    const uint32_t ref = word_ref(A::load(t.slots + slot));
    return ref & kInCall ? ref & ~kInCall : kKnown;
}

// After the outcome: a kept key i moves to place `at` of the key store and its slot refers to it.
template <class A>
KCDC_HD inline void commit_key(const Table& t, const Keys& call, uint32_t i, uint64_t slot, uint32_t at) {
    const uint64_t w = A::load(t.slots + slot);
    if (word_ref(w) != (kInCall | i)) return;  // not kept
    uint8_t* dst = t.store + uint64_t(at) * key_stride(t.id_len);  // 4-byte aligned
    const uint8_t* src = key_id(call, i);
    uint32_t b = 0;
    for (; b + 4u <= t.id_len; b += 4u) *reinterpret_cast<uint32_t*>(dst + b) = load32_any(src + b);
    for (; b < t.id_len; b++) dst[b] = src[b];
    dst[t.id_len] = key_prefix(call, i);
    A::store(t.slots + slot, slot_word(word_fp(w), at));
}

// Read-only probe: is key i of `q` in the set?
template <class A>
KCDC_HD inline bool probe_lookup(const Table& t, const Keys& q, uint32_t i) {
    const uint64_t h = key_hash(key_prefix(q, i), key_id(q, i));
    const uint32_t fp = fingerprint(h);
    for (uint64_t s = home_slot(h, t.nslots);; s = next_slot(s, t.nslots)) {
        const uint64_t w = A::load(t.slots + s);
        if (w == kEmpty) return false;
        if (word_matches(t, q, w, i, fp)) return true;
    }
}

}  // namespace dedupfmt

// ---- the launchers (kcdc_dedup.hip), called by kcdc_api.cpp after the parameter checks
struct DedupSet {
    int device;
    uint32_t id_len;
    uint64_t max_keys;
    uint8_t* base;  // one allocation, dedupfmt::layout
    uint32_t grid;  // workgroups of the persistent kernels: 16 waves per CU
};
int dedup_launch_clear(const DedupSet& t, void* stream);
// d_keep / d_first: nullptr for insert.  from: nullptr, or the set whose keys are inserted (grow).
int dedup_launch_claim(const DedupSet& t, const DedupSet* from, uint8_t prefix, const uint8_t* d_ids, uint32_t id_stride,
                       uint32_t n, uint8_t* d_keep, uint32_t* d_first, uint64_t* d_totals, void* stream);
int dedup_launch_lookup(const DedupSet& t, uint8_t prefix, const uint8_t* d_ids, uint32_t id_stride, uint32_t n,
                        uint8_t* d_known, void* stream);

}  // namespace kcdc
