// Every validity decision of the S2 decoder, for the device kernels (kcdc_decompress.hip) and the
// host program that runs the tests' vectors under the sanitizers (tools/s2_decode_host.cpp): the
// framing hop, the block's uvarint, each element's length, offset and bounds.  What
// s2.NewReader accepts (klauspost/compress/s2, the reader behind compressor_s2.go:73-90): the
// Snappy framing format, the Snappy block elements, and S2's repeat extension of copy-1.
// All arithmetic is on values bounded before they are added: a corrupt stream is refused by
// arithmetic, never survived by luck.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define KCDC_S2_HD __host__ __device__ inline
#else
#define KCDC_S2_HD inline
#endif

namespace kcdc {
namespace s2f {

constexpr uint32_t kMaxBlock = 4u << 20;  // S2's largest block (decoded bytes)
constexpr int32_t kBadMsg = -74, kOverflow = -75, kNoMem = -12;  // KCDC_EBADMSG, KCDC_EOVERFLOW, KCDC_ENOMEM
constexpr uint32_t kQuotaShift = 14;  // descriptors: one per content plus one per 16 KiB of its cap

KCDC_S2_HD uint32_t mask_crc(uint32_t c) { return ((c >> 15) | (c << 17)) + 0xa282ead8u; }

// One data chunk of a content: what the decode and CRC passes need.
struct Desc {
    uint64_t in_off;    // the payload after its CRC, from the start of the compressed buffer
    uint64_t out_off;   // the decoded bytes, from the start of the output buffer
    uint32_t in_len;    // payload bytes after the CRC
    uint32_t out_len;   // decoded bytes (<= kMaxBlock)
    uint32_t crc;       // the stored masked CRC-32C
    uint32_t content;   // bit 31: uncompressed chunk (0x01); the rest: the content's index
};
static_assert(sizeof(Desc) == 32, "Desc is 32 bytes");
constexpr uint32_t kDescRaw = 0x80000000u;

// uvarint in the little-endian bytes `b` (5 used at most), of which `avail` exist: 0 and *val, *used, or
// kBadMsg (runs past the input, longer than 5 bytes, or above kMaxBlock).
KCDC_S2_HD int32_t uvarint(uint64_t b, uint64_t avail, uint32_t* val, uint32_t* used) {
    uint64_t v = 0;
    for (uint32_t k = 0; k < 5; k++) {
        if (k >= avail) return kBadMsg;
        const uint32_t c = static_cast<uint32_t>(b >> (8u * k)) & 255u;
        v |= static_cast<uint64_t>(c & 127u) << (7u * k);
        if (!(c & 128u)) {
            if (v > kMaxBlock) return kBadMsg;
            *val = static_cast<uint32_t>(v);
            *used = k + 1u;
            return 0;
        }
    }
    return kBadMsg;
}

// The little-endian bytes p[i..i+5) that exist (others 0): the first argument of `uvarint` and
// `element` from plain memory.
KCDC_S2_HD uint64_t bytes_at(const uint8_t* p, uint64_t i, uint64_t n) {
    uint64_t b = 0;
    for (uint32_t k = 0; k < 5u && i + k < n; k++) b |= uint64_t(p[i + k]) << (8u * k);
    return b;
}

// The framing walk of one content p[0..n) = BE32(header ID) || S2 stream: every data chunk gets a
// descriptor in descs[0..max_desc), decoded lengths are summed against cap.  Returns the status
// (0, kBadMsg, kOverflow, kNoMem); on 0, *count descriptors describe *total decoded bytes.
// in_base / out_base: the content's and its slot's offsets in their buffers.
KCDC_S2_HD int32_t index_content(const uint8_t* p, uint64_t n, uint32_t header_id, uint64_t cap, uint32_t content,
                                 uint64_t in_base, uint64_t out_base, Desc* descs, uint64_t max_desc,
                                 uint32_t* count, uint64_t* total) {
    *count = 0;
    *total = 0;
    if (n < 4) return kBadMsg;  // verifyCompressionHeader
    const uint32_t id = (uint32_t(p[0]) << 24) | (uint32_t(p[1]) << 16) | (uint32_t(p[2]) << 8) | uint32_t(p[3]);
    if (id != header_id) return kBadMsg;
    uint64_t i = 4, o = 0;
    uint32_t k = 0;
    bool first = true;
    while (i < n) {
        if (n - i < 4) return kBadMsg;  // truncated chunk header
        const uint32_t type = p[i];
        const uint64_t len = uint64_t(p[i + 1]) | (uint64_t(p[i + 2]) << 8) | (uint64_t(p[i + 3]) << 16);
        i += 4;
        if (len > n - i) return kBadMsg;  // the chunk runs past the content
        const uint8_t* q = p + i;
        const uint64_t at = i;
        i += len;
        if (type == 0xffu) {  // stream identifier
            if (len != 6) return kBadMsg;
            const uint8_t s2[6] = {'S', '2', 's', 'T', 'w', 'O'}, sn[6] = {'s', 'N', 'a', 'P', 'p', 'Y'};
            bool is_s2 = true, is_sn = true;
            for (int j = 0; j < 6; j++) {
                is_s2 = is_s2 && q[j] == s2[j];
                is_sn = is_sn && q[j] == sn[j];
            }
            if (!is_s2 && !is_sn) return kBadMsg;
            first = false;
            continue;
        }
        if (first) return kBadMsg;  // the first chunk must be the identifier
        if (type >= 0x80u) continue;  // padding, index, skippable
        if (type >= 0x02u) return kBadMsg;  // reserved unskippable
        if (len < 4) return kBadMsg;
        uint32_t dec = 0, used = 0;
        if (type == 0x00u) {
            if (uvarint(bytes_at(q, 4, len), len - 4, &dec, &used) != 0) return kBadMsg;
        } else {
            if (len - 4 > kMaxBlock) return kBadMsg;
            dec = static_cast<uint32_t>(len - 4);
        }
        if (dec > cap - o) return kOverflow;  // o <= cap
        if (k >= max_desc) return kNoMem;
        Desc d;
        d.in_off = in_base + at + 4;
        d.out_off = out_base + o;
        d.in_len = static_cast<uint32_t>(len - 4);
        d.out_len = dec;
        d.crc = uint32_t(q[0]) | (uint32_t(q[1]) << 8) | (uint32_t(q[2]) << 16) | (uint32_t(q[3]) << 24);
        d.content = content | (type == 0x01u ? kDescRaw : 0u);
        descs[k++] = d;
        o += dec;
    }
    if (first) return kBadMsg;  // no identifier chunk at all
    *count = k;
    *total = o;
    return 0;
}

// One element of a block.
struct Elem {
    uint32_t hdr;   // tag and extra bytes
    uint32_t len;   // bytes it produces
    uint32_t off;   // copy: distance back (a repeat: the previous copy's); literal: 0
    bool copy;
};

// Parse and check the element whose bytes start with the little-endian `b` (the tag in its low
// byte, 5 bytes used at most; bytes past the input may hold anything).  avail: input bytes left
// from the tag on (>= 1); o: bytes decoded so far; want: the block's declared length (o <= want
// <= kMaxBlock); last_off: the previous copy's offset, 0 before the first.  0, or kBadMsg when the
// element runs past the input or the declared length, or its offset is 0 or reaches before the block.
KCDC_S2_HD int32_t element(uint64_t b, uint32_t avail, uint32_t o, uint32_t want, uint32_t last_off, Elem* e) {
    const uint32_t tag = static_cast<uint32_t>(b & 255u);
    const uint32_t x = static_cast<uint32_t>(b >> 8);  // the four bytes after the tag
    uint64_t len;
    uint32_t hdr, off = 0;
    switch (tag & 3u) {
        case 0: {
            const uint32_t f = tag >> 2;
            if (f < 60u) {
                hdr = 1;
                len = f + 1u;
            } else {
                const uint32_t nb = f - 59u;  // 1..4 length bytes
                hdr = 1u + nb;
                len = uint64_t(nb == 4u ? x : x & ((1u << (8u * nb)) - 1u)) + 1u;
            }
            if (hdr > avail || len > avail - hdr || len > want - o) return kBadMsg;
            e->hdr = hdr;
            e->len = static_cast<uint32_t>(len);
            e->off = 0;
            e->copy = false;
            return 0;
        }
        case 1: {
            const uint32_t l = (tag >> 2) & 7u;
            hdr = 2;
            len = 4u + l;
            off = ((tag >> 5) << 8) | (x & 255u);
            if (off == 0) {  // S2 repeat: the previous copy's offset, lengths 4..8 or extended
                off = last_off;
                if (l == 5u) {
                    hdr = 3;
                    len = 8u + ((x >> 8) & 0xffu);
                } else if (l == 6u) {
                    hdr = 4;
                    len = 260u + ((x >> 8) & 0xffffu);
                } else if (l == 7u) {
                    hdr = 5;
                    len = 65540u + (x >> 8);
                }
            }
            break;
        }
        case 2:
            hdr = 3;
            len = 1u + (tag >> 2);
            off = x & 0xffffu;
            break;
        default:
            hdr = 5;
            len = 1u + (tag >> 2);
            off = x;
            break;
    }
    if (hdr > avail || off == 0 || off > o || len > want - o) return kBadMsg;
    e->hdr = hdr;
    e->len = static_cast<uint32_t>(len);
    e->off = off;
    e->copy = true;
    return 0;
}

// One block in[0..n) (uvarint, elements) to out[0..want), byte by byte: the order of decisions the
// device's wave walk follows.  0 or kBadMsg.
KCDC_S2_HD int32_t decode_block_serial(const uint8_t* in, uint32_t n, uint8_t* out, uint32_t want) {
    uint32_t dec = 0, i = 0, o = 0, last_off = 0;
    if (uvarint(bytes_at(in, 0, n), n, &dec, &i) != 0 || dec != want) return kBadMsg;
    while (i < n) {
        Elem e;
        if (element(bytes_at(in, i, n), n - i, o, want, last_off, &e) != 0) return kBadMsg;
        if (e.copy) {
            for (uint32_t k = 0; k < e.len; k++) out[o + k] = out[o - e.off + k];
            last_off = e.off;
            i += e.hdr;
        } else {
            for (uint32_t k = 0; k < e.len; k++) out[o + k] = in[i + e.hdr + k];
            i += e.hdr + e.len;
        }
        o += e.len;
    }
    return o == want ? 0 : kBadMsg;
}

}  // namespace s2f
}  // namespace kcdc
