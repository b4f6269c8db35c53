// Every decision of kcdc_pack_chunks_device (kcdc_pack.hip), as functions the device kernels and
// the stand-alone host program tools/pack_plan_host.cpp both run: a content's status and stored
// size, the keep-or-drop rule, the placement of contents in packs (addToPackUnlocked,
// repo/content/content_manager.go:257-353) and the bounds of kcdc_pack_bounds.
#pragma once

#include <cstdint>

#include "kcdc_internal.h"  // KCDC_HD, the ECC geometry

namespace kcdc {
namespace packfmt {

constexpr uint32_t kSealOverhead = 28;                 // nonce(12) + tag(16), both encryptors
constexpr uint64_t kSealMaxLen = (1ull << 30) - 64;    // kcdc_encrypt_chunks_device: longer is KCDC_EFBIG
constexpr uint64_t kMaxPackSize = 1ull << 30;          // max_pack_size the call takes
constexpr uint64_t kMaxTotalBytes = 1ull << 40;        // max_total_bytes the call takes
constexpr uint64_t kPackAlign = 256;                   // pack k+1 starts at pack k's end rounded up to this
constexpr uint64_t kEccNoWrite = 1ull << 32;           // an ECC encode length that is refused and writes nothing
constexpr int32_t kPacked = 0, kSkipped = 1, kEfbig = -27, kEnomem = -12, kEoverflow = -75;

struct Rule {
    uint64_t max_pack_size;
    uint32_t lead, open_fill;
    uint32_t ecc;  // 0: none
    EccParams ep;
};

struct Row {  // kcdc_pack_info
    uint64_t start, length;
    uint32_t first, count;
};
struct Entry {  // kcdc_pack_entry
    uint32_t pack, pack_offset, packed_length, original_length, header_id;
    int32_t status;
};
struct Totals {
    uint64_t packs, bytes;
    int32_t refuse;  // 0 or kEoverflow
};

KCDC_HD inline uint64_t align_up(uint64_t x, uint64_t a) { return (x + a - 1) / a * a; }

// kcdc_compress_bound: BE32 header + 20 bytes of framing + the bytes + 5 per 512-byte segment
KCDC_HD inline uint64_t compress_bound(uint64_t len) { return 24u + len + 5u * ((len + 511u) / 512u); }

// Status of chunk i from its length and mask byte alone (before any capacity is known).
KCDC_HD inline int32_t chunk_status(uint64_t len, bool keep) {
    return !keep ? kSkipped : len > kSealMaxLen ? kEfbig : kPacked;
}

// maybeCompressAndEncryptDataForPacking, content_manager_lock_free.go:61-73: the compressed form
// (header included) is used only when it is shorter than the chunk.
KCDC_HD inline bool keep_compressed(uint64_t out_len, uint64_t len) { return out_len < len; }

// Bytes of pack a content of `plain` bytes (compressed or original) takes.
KCDC_HD inline uint64_t stored_size(const Rule& r, uint64_t plain) {
    const uint64_t sealed = plain + kSealOverhead;
    return r.ecc ? ecc_stored_size(ecc_geo_original(r.ep, sealed), sealed) : sealed;
}

// Length a pack has before its first content of this call.
KCDC_HD inline uint64_t pack_base(const Rule& r, uint64_t pack) {
    return pack == 0 && r.open_fill ? r.open_fill : r.lead;
}

// E[0..n]: exclusive prefix sums of the stored sizes (0 for a chunk that takes no room), E[n] the
// total.  The smallest j in [i, n) with E[j + 1] >= target, or n.
KCDC_HD inline uint32_t place_lower(const uint64_t* E, uint32_t n, uint32_t i, uint64_t target) {
    uint32_t lo = i, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (E[mid + 1] >= target) hi = mid;
        else lo = mid + 1u;
    }
    return lo;
}

// The sequential rule as a chain over the prefix sums: a pack opened before chunk i with base
// length c closes at the first j whose content brings it to max_pack_size, c + E[j + 1] - E[i] >=
// max_pack_size; the next opens at j + 1.  C: exclusive prefix counts of the chunks that take room.
KCDC_HD inline Totals place_chain(const Rule& r, const uint64_t* E, const uint64_t* C, uint32_t n, Row* rows,
                                  uint64_t rows_cap, uint64_t pack_cap) {
    Totals t{0, 0, 0};
    uint32_t i = 0;
    uint64_t start = 0;
    while (i < n && E[n] > E[i]) {
        const uint64_t c = pack_base(r, t.packs);
        const uint64_t need = r.max_pack_size > c ? r.max_pack_size - c : 1u;
        const uint32_t first = place_lower(E, n, i, E[i] + 1u);
        const uint32_t j = place_lower(E, n, first, E[i] + need);
        const uint32_t last = j < n ? j : n - 1u;
        const uint64_t length = c + (E[last + 1u] - E[i]);
        if (t.packs >= rows_cap || start + length > pack_cap) return Totals{0, 0, kEoverflow};
        rows[t.packs] = Row{start, length, first, static_cast<uint32_t>(C[last + 1u] - C[i])};
        t.packs++;
        t.bytes = start + length;
        start = align_up(start + length, kPackAlign);
        i = last + 1u;
    }
    return t;
}

// The pack of chunk i (one that takes room): the last row whose first chunk is not after i.
KCDC_HD inline uint32_t place_find(const Row* rows, uint32_t npacks, uint32_t i) {
    uint32_t lo = 0, hi = npacks;  // rows[lo].first <= i < rows[hi].first
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (rows[mid].first <= i) lo = mid;
        else hi = mid;
    }
    return lo;
}

// The entry of chunk i once the chain is known.  `refuse`: the call-wide refusal, or 0.
KCDC_HD inline Entry place_entry(const Rule& r, const uint64_t* E, const Row* rows, uint32_t npacks, uint32_t i,
                                 uint64_t len, int32_t status, uint32_t header_id, int32_t refuse) {
    Entry e{0, 0, 0, static_cast<uint32_t>(len), 0, refuse ? refuse : status};
    if (e.status != kPacked) return e;
    e.pack = place_find(rows, npacks, i);
    e.pack_offset = static_cast<uint32_t>(pack_base(r, e.pack) + (E[i] - E[rows[e.pack].first]));
    e.packed_length = static_cast<uint32_t>(E[i + 1u] - E[i]);
    e.header_id = header_id;
    return e;
}

// ---- bounds (kcdc_pack_bounds): what n chunks of at most `total` bytes in all can need
// Stored bytes in all.  Without ECC total + 28 n.  With ECC, for x = sealed length + 4:
//   6+2 code      8 (ceil(x / 6) + 4)                      <= 4 x / 3 + 39
//   one block     (D + P)(ceil(x / D) + 4), x > 8 (D + P)   <= x ((D + P) / D + 5 / 8)
//   many blocks   ceil(x / (D S)) P (S + 4) + x + 4 ceil(x / S), x > D S
//                                                           <= x (1 + 4 / S + 2 P (S + 4) / (D S)) + 4
// so stored <= x R + 44 with R the largest of the three factors (in thousandths, rounded up).
KCDC_HD inline uint64_t stored_bound(const Rule& r, uint64_t total, uint32_t n) {
    if (!r.ecc) return total + uint64_t(kSealOverhead) * n;
    const uint64_t D = r.ep.data, P = r.ep.parity, S = r.ep.max_shard;
    uint64_t f = 1334;
    const uint64_t f1 = (1000u * (D + P) + D - 1u) / D + 625u;
    const uint64_t f2 = 1000u + (4000u + S - 1u) / S + (2000u * P * (S + 4u) + D * S - 1u) / (D * S);
    if (f1 > f) f = f1;
    if (f2 > f) f = f2;
    const uint64_t x = total + uint64_t(kSealOverhead + kEccLengthSize) * n;
    return x / 1000u * f + (x % 1000u * f + 999u) / 1000u + 44ull * n;
}

// Packs: every closed pack but the first holds at least max(28, max_pack_size - lead) stored bytes.
KCDC_HD inline uint64_t packs_bound(const Rule& r, uint64_t stored, uint32_t n) {
    uint64_t q = r.max_pack_size > r.lead ? r.max_pack_size - r.lead : 1u;
    if (q < kSealOverhead) q = kSealOverhead;
    const uint64_t p = 2u + stored / q;
    return p < n ? p : n;
}
KCDC_HD inline uint64_t pack_bytes_bound(const Rule& r, uint64_t stored, uint64_t packs) {
    return stored + packs * (uint64_t(r.lead) + kPackAlign - 1u) + r.open_fill;
}

// ---- workspace of kcdc_pack_chunks_device (offsets from a 256-byte aligned d_work)
struct Ws {
    uint64_t scal, wlen, comp_off, comp_len, stage_off, seal_off, seal_len, E, C, dst_off, aux, comp_ids, seal_st,
        ecc_st, comp_area, stage_area, comp_ws, crypt_ws, total;
};
constexpr uint32_t kScalars = 8;  // u64: [0] sum of the kept lengths, [1] refusal, [2] packs, [3] gather ticket
inline Ws ws_layout(uint32_t n, uint64_t total, bool comp, uint64_t comp_ws_bytes, uint64_t crypt_ws_bytes) {
    Ws w{};
    uint64_t at = 0;
    auto take = [&](uint64_t bytes) {
        const uint64_t o = at;
        at = align_up(at + bytes, 256);
        return o;
    };
    const uint64_t a8 = (uint64_t(n) + 1u) * 8u, a4 = uint64_t(n) * 4u;
    w.scal = take(kScalars * 8u);
    w.wlen = take(a8);
    w.comp_off = take(a8);
    w.comp_len = take(a8);
    w.stage_off = take(a8);
    w.seal_off = take(a8);
    w.seal_len = take(a8);
    w.E = take(a8);
    w.C = take(a8);
    w.dst_off = take(a8);
    w.aux = take(a8);
    w.comp_ids = take(a4);
    w.seal_st = take(a4);
    w.ecc_st = take(a4);
    // compress slots: the sum of compress_bound over lengths that sum to at most `total`
    w.comp_area = take(comp ? 29ull * n + total + 5u * (total / 512u) + 16u : 0u);
    // sealed staging slots: align4(len + 28) each
    w.stage_area = take(total + 31ull * n + 16u);
    w.comp_ws = take(comp ? comp_ws_bytes : 0u);
    w.crypt_ws = take(crypt_ws_bytes);
    w.total = at;
    return w;
}

}  // namespace packfmt

// ---- the launcher (kcdc_pack.hip), called by kcdc_api.cpp after the parameter checks
struct PackRun {
    packfmt::Rule rule;
    const char *compression, *encryption, *ecc;  // compression / ecc: nullptr for none
    const uint8_t* secret;
    uint32_t secret_len;
    int32_t ecc_overhead, ecc_max_shard;
    uint64_t max_total;
};
uint64_t pack_workspace_size(const PackRun& r, uint32_t nchunks);
int launch_pack(const PackRun& r, const uint8_t* d_data, const uint64_t* d_offsets, const uint64_t* d_lens,
                const uint8_t* d_keep, uint32_t nchunks, const uint8_t* d_ids, uint32_t id_len, uint32_t id_stride,
                const uint8_t* d_nonces, uint8_t* d_pack, uint64_t pack_cap, void* d_entries, void* d_packs,
                uint32_t packs_cap, uint64_t* d_totals, void* d_work, uint64_t work_bytes, void* stream);

}  // namespace kcdc
