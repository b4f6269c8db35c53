// Every decision the zstd decoder takes on untrusted bytes, for the device kernels (kcdc_zstd.hip)
// and the host program that runs the tests' vectors under the sanitizers
// (tools/zstd_decode_host.cpp): the header ID, the RFC 8878 frame and block hop, the literals and
// sequences section headers, the Huffman weight and FSE description parsers with their bounded
// table builds, the code-to-value tables, the repeat-offset rule, the sequence executor's batch
// logic with every bound on input, output and room, and XXH64.  What the reference's reader accepts
// (compressor_zstd.go:73-91: verifyCompressionHeader, then klauspost/compress/zstd.NewReader).
//
// The decoder is written once, over an `Io` that says which lane of how many is running, orders
// the lanes (sync, fence) and copies.  The host Io is one lane over exactly-sized heap buffers; the
// device Io is one wave.  Serial steps (headers, table builds, the FSE state walk, the batch plan)
// are run by the leader lane alone and handed to the others through a context in LDS.  All lengths
// are compared against what is left and never added first; every loop over input is bounded by a
// count known before it starts.
//
// Choices where readers differ or the format is silent.  Go's behaviour is followed where
// klauspost/compress's published source settles it (that library is not available to the tests, so
// no test rests on it); otherwise RFC 8878 and libzstd:
//  * a match offset beyond the bytes the *frame* has produced is refused, and so is one beyond
//    Window_Size: a later frame never reaches into an earlier one (RFC 8878 3.1.1.1.1.2; libzstd's
//    one-shot decoder checks the first and not the second: stricter here);
//  * a Dictionary_ID field is accepted only when its value is 0; any other value is KCDC_EBADMSG,
//    because no dictionary exists here (libzstd decodes such a frame without the dictionary);
//  * a content with no frame at all (the 4-byte header ID alone) decodes to 0 bytes (libzstd's
//    ZSTD_decompress returns 0 for an empty source; io.Copy over an empty reader copies nothing);
//  * a Compressed_Block of 2 bytes (an empty Raw literals section and Number_of_Sequences 0) is
//    accepted as the RFC allows and Go's blockDec does (`len(in) < 2`); libzstd wants 3;
//  * a Compressed_Block of 128 KiB or more is refused (libzstd: srcSize >= ZSTD_BLOCKSIZE_MAX; the
//    RFC asks a compressed block to be smaller than what it decodes to);
//  * a block that decodes to more than Block_Maximum_Size = min(Window_Size, 128 KiB) is refused
//    (RFC 8878 3.1.1.2.4; libzstd's one-shot decoder does not check a compressed block's);
//  * Huffman weights must give at least two symbols of weight 1, and an even number of them
//    (libzstd's HUF_readStats and huff0's ReadTable both refuse otherwise), codes are at most 11
//    bits (RFC 8878 4.2.1 and huff0's tableLogMax; libzstd 1.4.8 decodes a complete 12-bit code),
//    and the FSE description of the weights may name up to 256 symbols;
//  * Repeat_Mode names the table of the last block *of the frame* with sequences whose mode was not
//    Repeat_Mode (Predefined, RLE or FSE_Compressed alike), Treeless literals the last Compressed
//    literals of the frame; without one the block is refused (libzstd: fseEntropy / litEntropy);
//  * the Unused_Bit of the frame header descriptor is ignored, the Reserved_Bit refused;
//  * every Window_Descriptor is accepted, exponents up to 31 + 10 included; a Window_Size above
//    2^32 - 1 counts as 2^32 - 1, which no offset of a content below 4 GiB can pass (libzstd refuses
//    a windowLog over 31, or over 27 unless told otherwise, and Go's reader has a configurable
//    maximum: both are limits on memory, and this decoder keeps no window);
//  * a raw or RLE block over Block_Maximum_Size is refused like a compressed one (RFC 8878
//    3.1.1.2.3; libzstd 1.4.8's one-shot decoder holds neither to it);
//  * the two reserved bits of the Symbol_Compression_Modes byte must be 0 (RFC 8878 3.1.1.3.2.1 and
//    Go's blockDec; libzstd ignores them);
//  * every backward bit stream must be consumed exactly, the sequences' as well as the literals'
//    and the weights' (Go's sequence decoder refuses extra bits; libzstd 1.4.8 checks the Huffman
//    streams only);
//  * the offset 0 that repeat code 3 with Literals_Length 0 gives when the first repeat offset
//    is 1 is refused, as RFC 8878 3.1.1.5 has it (libzstd forces such an offset to 1);
//  * the first three streams of a 4-stream literals section regenerate (size + 3) / 4 bytes each;
//    a size for which three of those exceed the whole is refused;
//  * a Treeless or Repeat_Mode block more than 2^26 - 1 blocks after the block that carries its
//    table gets KCDC_ENOMEM: a descriptor cannot name a carrier further back (this needs 2 GiB of
//    descriptor room, far beyond what the workspace rule grants any content below 4 GiB).
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define KCDC_ZS_HD __host__ __device__ __forceinline__  // no call keeps a header struct in private memory
#else
#define KCDC_ZS_HD inline
#endif

#ifndef KCDC_ZSTD_BATCH
#define KCDC_ZSTD_BATCH 64
#endif

namespace kcdc {
namespace zsf {

constexpr int32_t kBadMsg = -74, kOverflow = -75, kNoMem = -12;  // KCDC_EBADMSG, KCDC_EOVERFLOW, KCDC_ENOMEM

constexpr uint32_t kZstdBatch = KCDC_ZSTD_BATCH;  // sequences the executor plans and copies at once (1: the serial walk)
static_assert(kZstdBatch >= 1 && kZstdBatch <= 64, "a batch is at most a wave of sequences");

constexpr uint32_t kBlockMax = 131072;                    // Block_Maximum_Size's ceiling
constexpr uint32_t kHufLog = 11;                          // longest Huffman code
constexpr uint32_t kLLLog = 9, kOFLog = 8, kMLLog = 9;    // accuracy-log limits of the sequence tables
constexpr uint32_t kWLog = 6;                             // ... and of the weights' table
constexpr uint32_t kLLMax = 35, kOFMax = 31, kMLMax = 52; // largest symbol of each
constexpr uint32_t kQuotaShift = 10, kQuotaBase = 4;      // descriptors per content: 4 + cap / 1 KiB
constexpr uint32_t kCarrierBits = 26;

KCDC_ZS_HD uint32_t le16(const uint8_t* p) { return p[0] | (uint32_t(p[1]) << 8); }
KCDC_ZS_HD uint32_t le24(const uint8_t* p) { return le16(p) | (uint32_t(p[2]) << 16); }
KCDC_ZS_HD uint32_t le32(const uint8_t* p) { return le16(p) | (le16(p + 2) << 16); }
KCDC_ZS_HD uint64_t le64(const uint8_t* p) { return le32(p) | (uint64_t(le32(p + 4)) << 32); }
KCDC_ZS_HD uint32_t highbit(uint32_t v) {  // v != 0
    uint32_t r = 0;
    while (v >>= 1) r++;
    return r;
}

// ---------------------------------------------------------------- descriptors
// One 32-byte descriptor per block, and one per frame in front of the frame's blocks.  Fields are
// bit ranges of the 256 bits: (position, width).
struct Desc {
    uint64_t q[4];
};
struct Field {
    uint32_t pos, width;
};
constexpr Field kFInOff{0, 32};     // block: its content's place in the content's bytes; frame: kFrame* flags
constexpr Field kFInLen{32, 18};    // Block_Size
constexpr Field kFType{50, 3};      // 0 raw, 1 RLE, 2 compressed, 4 frame
constexpr Field kFLast{53, 1};      // last block of its frame
constexpr Field kFRegen{54, 18};    // compressed: the literals' regenerated size
constexpr Field kFNseq{72, 17};     // compressed: Number_of_Sequences
constexpr Field kFLitPos{89, 32};   // compressed: place in the content's literal room
constexpr Field kFSeqPos{121, 31};  // compressed: place in the content's sequence room
constexpr Field kFHufC{152, 26};    // blocks back to the carrier of the Huffman code (Treeless)
constexpr Field kFLLC{178, 26};     // ... of the LL, OF and ML tables (Repeat_Mode)
constexpr Field kFOFC{204, 26};
constexpr Field kFMLC{230, 26};
constexpr uint32_t kTypeRaw = 0, kTypeRle = 1, kTypeComp = 2, kTypeFrame = 4;
constexpr uint32_t kFrameHasSize = 1, kFrameHasSum = 2;
// A frame's descriptor: q[1] = Frame_Content_Size (low 32 bits; a larger one is over every cap) |
// stored checksum << 32; q[2] = Window_Size (clamped to 32 bits) | first output byte << 32 (the
// execute pass writes it); q[3] = decoded bytes (the execute pass writes it).

// The words are picked by comparisons, not by indexing: a descriptor held in registers stays there.
KCDC_ZS_HD uint64_t dword(const Desc& d, uint32_t i) { return i == 0 ? d.q[0] : i == 1u ? d.q[1] : i == 2u ? d.q[2] : d.q[3]; }
KCDC_ZS_HD uint64_t dget(const Desc& d, Field f) {
    const uint32_t i = f.pos >> 6, s = f.pos & 63u;
    uint64_t v = dword(d, i) >> s;
    if (s + f.width > 64u) v |= dword(d, i + 1u) << (64u - s);
    return v & ((uint64_t(1) << f.width) - 1u);
}
KCDC_ZS_HD void dput(Desc& d, Field f, uint64_t v) {  // into zeroed bits
    const uint32_t i = f.pos >> 6, s = f.pos & 63u;
    for (uint32_t k = 0; k < 4u; k++) {
        if (k == i) d.q[k] |= v << s;
        if (k == i + 1u && s + f.width > 64u) d.q[k] |= v >> (64u - s);
    }
}

struct SeqRec {  // one decoded sequence: 12 bytes, no limit on any field the format allows
    uint32_t ll, ml, ofv;  // Literals_Length, Match_Length, Offset_Value (1..3: repeat codes)
};

// ---------------------------------------------------------------- section headers
struct Frame {
    uint64_t fcs, window;
    uint32_t has_fcs, checksum, hdr_len;
};
// The frame header after its magic: 0, or kBadMsg.
KCDC_ZS_HD int32_t frame_header(const uint8_t* p, uint32_t left, Frame* f) {
    if (left < 1u) return kBadMsg;
    const uint32_t fhd = p[0];
    const uint32_t fcs_flag = fhd >> 6, single = (fhd >> 5) & 1u, did_flag = fhd & 3u;
    if (fhd & 8u) return kBadMsg;  // Reserved_Bit
    f->checksum = (fhd >> 2) & 1u;
    uint32_t pos = 1;
    f->window = 0;
    if (!single) {
        if (left - pos < 1u) return kBadMsg;
        const uint32_t wd = p[pos++];
        const uint64_t base = uint64_t(1) << (10u + (wd >> 3));
        f->window = base + (base >> 3) * (wd & 7u);
    }
    const uint32_t did_len = did_flag == 3u ? 4u : did_flag;
    if (left - pos < did_len) return kBadMsg;
    for (uint32_t k = 0; k < did_len; k++)
        if (p[pos + k] != 0) return kBadMsg;  // no dictionary exists here
    pos += did_len;
    const uint32_t fcs_len = fcs_flag == 0 ? single : fcs_flag == 1u ? 2u : fcs_flag == 2u ? 4u : 8u;
    if (left - pos < fcs_len) return kBadMsg;
    f->has_fcs = fcs_len != 0;
    f->fcs = 0;
    if (fcs_len == 1u) f->fcs = p[pos];
    if (fcs_len == 2u) f->fcs = le16(p + pos) + 256u;
    if (fcs_len == 4u) f->fcs = le32(p + pos);
    if (fcs_len == 8u) f->fcs = le64(p + pos);
    pos += fcs_len;
    if (single) f->window = f->fcs;
    f->hdr_len = pos;
    return 0;
}

struct LitHdr {
    uint32_t type, regen, comp, streams, hlen, body;  // body: the section's bytes after its header
};
// The literals section header of a block's `left` bytes: 0, or kBadMsg.
KCDC_ZS_HD int32_t lit_header(const uint8_t* p, uint32_t left, LitHdr* h) {
    if (left < 1u) return kBadMsg;
    const uint32_t b0 = p[0], sf = (b0 >> 2) & 3u;
    h->type = b0 & 3u;
    h->comp = 0;
    h->streams = 1;
    if (h->type < 2u) {  // Raw, RLE
        h->hlen = sf == 1u ? 2u : sf == 3u ? 3u : 1u;
        if (left < h->hlen) return kBadMsg;
        h->regen = h->hlen == 1u ? b0 >> 3 : h->hlen == 2u ? le16(p) >> 4 : le24(p) >> 4;
        h->body = h->type == 0 ? h->regen : 1u;
    } else {  // Compressed, Treeless
        h->hlen = sf < 2u ? 3u : sf + 2u;
        if (left < h->hlen) return kBadMsg;
        h->streams = sf == 0 ? 1u : 4u;
        if (h->hlen == 3u) {
            const uint32_t v = le24(p);
            h->regen = (v >> 4) & 0x3ffu;
            h->comp = v >> 14;
        } else if (h->hlen == 4u) {
            const uint32_t v = le32(p);
            h->regen = (v >> 4) & 0x3fffu;
            h->comp = v >> 18;
        } else {
            const uint64_t v = le32(p) | (uint64_t(p[4]) << 32);
            h->regen = static_cast<uint32_t>(v >> 4) & 0x3ffffu;
            h->comp = static_cast<uint32_t>(v >> 22);
        }
        h->body = h->comp;
    }
    if (h->regen > kBlockMax) return kBadMsg;
    if (h->body > left - h->hlen) return kBadMsg;
    return 0;
}

struct SeqHdr {
    uint32_t nseq, hlen, modes;  // the modes byte: LL, OF, ML from the top, 0 Predefined, 1 RLE, 2 FSE_Compressed, 3 Repeat
};
KCDC_ZS_HD uint32_t seq_mode(const SeqHdr& h, uint32_t t) { return (h.modes >> (6u - 2u * t)) & 3u; }
KCDC_ZS_HD int32_t seq_header(const uint8_t* p, uint32_t left, SeqHdr* h) {
    if (left < 1u) return kBadMsg;
    const uint32_t b0 = p[0];
    h->modes = 0;
    if (b0 < 128u) {
        h->nseq = b0;
        h->hlen = 1;
    } else if (b0 < 255u) {
        if (left < 2u) return kBadMsg;
        h->nseq = ((b0 - 128u) << 8) + p[1];
        h->hlen = 2;
    } else {
        if (left < 3u) return kBadMsg;
        h->nseq = le16(p + 1) + 0x7F00u;
        h->hlen = 3;
    }
    if (h->nseq == 0) return h->hlen == left ? 0 : kBadMsg;  // nothing may follow
    if (left - h->hlen < 1u) return kBadMsg;
    const uint32_t m = p[h->hlen++];
    if (m & 3u) return kBadMsg;  // reserved
    h->modes = m;
    return 0;
}

// ---------------------------------------------------------------- bit streams
// A forward little-endian bit reader over p[0..n) (FSE descriptions).
struct FwdBits {
    const uint8_t* p;
    uint32_t n, bit;  // bit: consumed so far
    bool over;
};
KCDC_ZS_HD uint32_t fwd_peek(const FwdBits& b, uint32_t nb) {  // nb <= 16; bits past the end are zeros
    const uint32_t i = b.bit >> 3;
    uint32_t v = 0;
    for (uint32_t k = 0; k < 3u; k++)
        if (i + k < b.n) v |= uint32_t(b.p[i + k]) << (8u * k);
    return (v >> (b.bit & 7u)) & ((1u << nb) - 1u);
}
KCDC_ZS_HD void fwd_skip(FwdBits& b, uint32_t nb) {
    b.bit += nb;
    if (b.bit > 8u * b.n) b.over = true;
}

// The backward bit stream of s[0..n): its last byte holds the final-bit marker; bits are taken from
// the marker down.  Reading below bit 0 gives zeros and leaves pos negative: such a stream fails
// the exact-consumption check at its end.
struct BackBits {
    const uint8_t* s;
    int64_t pos;    // bits left: the next one is bit pos - 1
    int64_t wbase;  // win holds bits [wbase, wbase + 64)
    uint64_t win;
};
KCDC_ZS_HD bool back_init(BackBits& b, const uint8_t* s, uint32_t n) {
    if (n == 0 || s[n - 1] == 0) return false;
    b.s = s;
    b.pos = int64_t(8) * (n - 1u) + highbit(s[n - 1]);
    b.wbase = b.pos + 1;  // nothing held
    b.win = 0;
    return true;
}
KCDC_ZS_HD uint32_t back_peek(BackBits& b, uint32_t nb) {  // nb <= 32
    if (nb == 0 || b.pos <= 0) return 0;
    const int64_t lo = b.pos - nb;
    if (lo < b.wbase || b.pos > b.wbase + 64) {
        const int64_t end = (b.pos + 7) >> 3;  // bytes [end - 8, end), those before the stream zeros
        uint64_t w = 0;
        for (int64_t k = 0; k < 8; k++) {
            const int64_t i = end - 8 + k;
            if (i >= 0) w |= uint64_t(b.s[i]) << (8 * k);
        }
        b.win = w;
        b.wbase = 8 * end - 64;
    }
    return static_cast<uint32_t>((b.win >> (lo - b.wbase)) & ((uint64_t(1) << nb) - 1u));
}
KCDC_ZS_HD uint32_t back_read(BackBits& b, uint32_t nb) {
    const uint32_t v = back_peek(b, nb);
    b.pos -= nb;
    return v;
}

// ---------------------------------------------------------------- FSE
// The normalized counts of an FSE description at p[0..left): norm[0..*nsym), -1 for "less than 1".
// 0 with *used its bytes, or kBadMsg.  norm holds max_sym + 1 entries.
KCDC_ZS_HD int32_t fse_read(const uint8_t* p, uint32_t left, uint32_t max_log, uint32_t max_sym, int16_t* norm,
                            uint32_t* nsym, uint32_t* log, uint32_t* used) {
    FwdBits b{p, left, 0, false};
    const uint32_t al = fwd_peek(b, 4) + 5u;
    fwd_skip(b, 4);
    if (al > max_log) return kBadMsg;
    int32_t remaining = (1 << al) + 1, threshold = 1 << al;
    uint32_t nb = al + 1u, sym = 0;
    while (remaining > 1 && sym <= max_sym) {  // at most max_sym + 1 rounds
        const int32_t max = (2 * threshold - 1) - remaining;
        int32_t count;
        const int32_t low = static_cast<int32_t>(fwd_peek(b, nb - 1u));
        if (low < max) {
            count = low;
            fwd_skip(b, nb - 1u);
        } else {
            count = static_cast<int32_t>(fwd_peek(b, nb));
            if (count >= threshold) count -= max;
            fwd_skip(b, nb);
        }
        count--;  // -1: less than 1
        // No count can overfill the table: the short form gives count + 1 < max <= remaining - 1
        // (threshold <= remaining), the long form at most 2 * threshold - 1 - max = remaining, so
        // count <= remaining - 1 either way and remaining stays >= 1.  The encoding has no word
        // for an over-full description; one that falls short is refused after the loop.
        remaining -= count < 0 ? 1 : count;
        norm[sym++] = static_cast<int16_t>(count);
        if (count == 0) {  // zero-repeat flags: each adds up to 3 more zeros, 3 asks for another flag
            for (;;) {
                const uint32_t r = fwd_peek(b, 2);
                fwd_skip(b, 2);
                if (r > max_sym + 1u - sym) return kBadMsg;  // sym <= max_sym + 1: the run ends the loop
                for (uint32_t k = 0; k < r; k++) norm[sym++] = 0;
                if (r != 3u || b.over) break;
            }
        }
        if (b.over) return kBadMsg;
        while (remaining < threshold) {
            nb--;
            threshold >>= 1;
        }
    }
    if (remaining != 1 || b.over) return kBadMsg;
    *nsym = sym;
    *log = al;
    *used = (b.bit + 7u) >> 3;
    return 0;
}

// A decoding table entry: symbol | bits to read << 8 | baseline << 16.
KCDC_ZS_HD uint32_t fe_sym(uint32_t e) { return e & 255u; }
KCDC_ZS_HD uint32_t fe_bits(uint32_t e) { return (e >> 8) & 255u; }
KCDC_ZS_HD uint32_t fe_base(uint32_t e) { return e >> 16; }

// The decoding table of norm[0..nsym) (their magnitudes sum to 1 << log, log <= the table's room)
// into tab[0..1 << log).  next: nsym entries of scratch.  0, or kBadMsg.
KCDC_ZS_HD int32_t fse_build(const int16_t* norm, uint32_t nsym, uint32_t log, uint32_t* tab, uint16_t* next) {
    const uint32_t size = 1u << log, mask = size - 1u;
    uint32_t high = size;  // cells [high, size) hold the less-than-1 symbols
    for (uint32_t s = 0; s < nsym; s++) {
        if (norm[s] == -1) {
            if (high == 0) return kBadMsg;
            tab[--high] = s;
            next[s] = 1;
        } else {
            next[s] = static_cast<uint16_t>(norm[s]);
        }
    }
    const uint32_t step = (size >> 1) + (size >> 3) + 3u;
    uint32_t pos = 0, placed = 0;
    for (uint32_t s = 0; s < nsym; s++) {
        for (int32_t i = 0; i < norm[s]; i++) {
            if (placed++ >= high) return kBadMsg;  // more cells than the table has (fse_read rules it out)
            tab[pos] = s;
            do pos = (pos + step) & mask;
            while (pos >= high);
        }
    }
    if (placed != high) return kBadMsg;
    for (uint32_t u = 0; u < size; u++) {
        const uint32_t s = tab[u], ns = next[s]++;
        const uint32_t nb = log - highbit(ns);
        tab[u] = s | (nb << 8) | (((ns << nb) - size) << 16);
    }
    return 0;
}

// RFC 8878 3.1.1.3.2.2: the predefined distributions.
KCDC_ZS_HD int32_t predefined(uint32_t t, int16_t* norm, uint32_t* nsym, uint32_t* log) {
    static constexpr int8_t ll[36] = {4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2,
                                      2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1};
    static constexpr int8_t of[29] = {1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1};
    static constexpr int8_t ml[53] = {1, 4, 3, 2, 2, 2, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1,
                                      1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1, -1, -1};
    const uint32_t n = t == 0 ? 36u : t == 1u ? 29u : 53u;
    for (uint32_t s = 0; s < n; s++) norm[s] = t == 0 ? ll[s] : t == 1u ? of[s] : ml[s];
    *nsym = n;
    *log = t == 1u ? 5u : 6u;
    return 0;
}

// Code to value (RFC 8878 3.1.1.3.2.1.1): baseline and extra bits.
KCDC_ZS_HD uint32_t ll_base(uint32_t c) {
    static constexpr uint32_t v[36] = {0,  1,  2,  3,  4,  5,  6,  7,  8,   9,   10,  11,   12,   13,   14,   15,    16,    18,
                                       20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536};
    return v[c];
}
KCDC_ZS_HD uint32_t ll_bits(uint32_t c) {
    static constexpr uint8_t v[36] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1,
                                      1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16};
    return v[c];
}
KCDC_ZS_HD uint32_t ml_base(uint32_t c) {
    static constexpr uint32_t v[21] = {35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099, 8195, 16387, 32771, 65539};
    return c < 32u ? c + 3u : v[c - 32u];
}
KCDC_ZS_HD uint32_t ml_bits(uint32_t c) {
    static constexpr uint8_t v[21] = {1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16};
    return c < 32u ? 0u : v[c - 32u];
}

// ---------------------------------------------------------------- Huffman
// The weights of a Huffman tree description at p[0..left) into w[0..*nsym) (the implied last one
// included), the code's longest length into *bits and the description's bytes into *used.
// ftab: 1 << kWLog entries, next / norm: 256 entries of scratch.  0, or kBadMsg.
KCDC_ZS_HD int32_t huf_weights(const uint8_t* p, uint32_t left, uint8_t* w, uint32_t* nsym, uint32_t* bits,
                               uint32_t* used, uint32_t* ftab, uint16_t* next, int16_t* norm) {
    if (left < 1u) return kBadMsg;
    const uint32_t hb = p[0];
    uint32_t n = 0;
    if (hb >= 128u) {  // direct: 4 bits each
        n = hb - 127u;
        const uint32_t bytes = (n + 1u) >> 1;
        if (left - 1u < bytes) return kBadMsg;
        for (uint32_t i = 0; i < n; i++) w[i] = (i & 1u) ? p[1u + (i >> 1)] & 15u : p[1u + (i >> 1)] >> 4;
        *used = 1u + bytes;
    } else {  // FSE-compressed: hb bytes, two interleaved states
        if (hb == 0 || left - 1u < hb) return kBadMsg;
        uint32_t fn = 0, flog = 0, fused = 0;
        if (fse_read(p + 1, hb, kWLog, 255u, norm, &fn, &flog, &fused) != 0) return kBadMsg;
        if (fse_build(norm, fn, flog, ftab, next) != 0) return kBadMsg;
        BackBits b;
        if (fused >= hb || !back_init(b, p + 1u + fused, hb - fused)) return kBadMsg;
        uint32_t s1 = back_read(b, flog), s2 = back_read(b, flog);
        if (b.pos < 0) return kBadMsg;
        for (;;) {  // at most 255 weights
            if (n > 253u) return kBadMsg;
            w[n++] = static_cast<uint8_t>(fe_sym(ftab[s1]));
            s1 = fe_base(ftab[s1]) + back_read(b, fe_bits(ftab[s1]));
            if (b.pos < 0) {
                w[n++] = static_cast<uint8_t>(fe_sym(ftab[s2]));
                break;
            }
            if (n > 253u) return kBadMsg;
            w[n++] = static_cast<uint8_t>(fe_sym(ftab[s2]));
            s2 = fe_base(ftab[s2]) + back_read(b, fe_bits(ftab[s2]));
            if (b.pos < 0) {
                w[n++] = static_cast<uint8_t>(fe_sym(ftab[s1]));
                break;
            }
        }
        *used = 1u + hb;
    }
    uint32_t sum = 0;
    for (uint32_t i = 0; i < n; i++) {
        if (w[i] > kHufLog) return kBadMsg;
        if (w[i]) sum += 1u << (w[i] - 1u);
    }
    if (sum == 0) return kBadMsg;
    const uint32_t log = highbit(sum) + 1u;
    if (log > kHufLog) return kBadMsg;
    const uint32_t rest = (1u << log) - sum;
    if (rest & (rest - 1u)) return kBadMsg;  // the weights do not complete a power of two
    w[n++] = static_cast<uint8_t>(highbit(rest) + 1u);
    uint32_t ones = 0;
    for (uint32_t i = 0; i < n; i++) ones += w[i] == 1u;
    if (ones < 2u || (ones & 1u)) return kBadMsg;
    *nsym = n;
    *bits = log;
    return 0;
}

// The decoding table of the weights: tab[0..1 << bits), an entry = symbol | code length << 8.
KCDC_ZS_HD void huf_build(const uint8_t* w, uint32_t nsym, uint32_t bits, uint16_t* tab) {
    uint32_t pos = 0;
    for (uint32_t wt = 1; wt <= bits; wt++) {  // longest codes first, symbols in order
        const uint32_t span = 1u << (wt - 1u), len = bits + 1u - wt;
        for (uint32_t s = 0; s < nsym; s++) {
            if (w[s] != wt) continue;
            for (uint32_t k = 0; k < span && pos < (1u << bits); k++) tab[pos++] = static_cast<uint16_t>(s | (len << 8));
        }
    }
}

// One Huffman stream s[0..n) into dst[0..count): 0, or kBadMsg (no marker, not consumed exactly).
KCDC_ZS_HD int32_t huf_stream(const uint8_t* s, uint32_t n, const uint16_t* tab, uint32_t bits, uint8_t* dst,
                              uint32_t count) {
    BackBits b;
    if (!back_init(b, s, n)) return kBadMsg;
    for (uint32_t i = 0; i < count; i++) {
        const uint32_t e = tab[back_peek(b, bits)];  // below the stream's first bit: zeros
        dst[i] = static_cast<uint8_t>(e);
        b.pos -= e >> 8;
    }
    return b.pos == 0 ? 0 : kBadMsg;
}

// ---------------------------------------------------------------- the entropy pass of one block
// What a wave (or the host) holds while it decodes a block: the tables and the build scratch.
// 10,084 bytes.
struct Ctx {
    uint16_t huf[1u << kHufLog];
    uint32_t llt[1u << kLLLog], oft[1u << kOFLog], mlt[1u << kMLLog];
    int16_t norm[256];
    uint8_t w[256];      // Huffman weights; the sequence tables' build scratch after them
    uint32_t log[3];     // accuracy logs of llt, oft, mlt as built
    uint32_t huf_bits;
    int32_t status;
    uint32_t s_off[4], s_len[4], s_out[4], s_cnt[4], nstreams;  // the literal streams: place, bytes, output place, symbols
    uint32_t lit_type, lit_byte, seq_at;
};

static_assert(sizeof(Ctx) == 10084, "the entropy context leaves 16 waves per CU their LDS");
static_assert(sizeof(Desc) == 32 && sizeof(SeqRec) == 12, "the workspace rule counts 32-byte descriptors and 12-byte records");

// Where table t's description of a block starts: walks the block's sections as the entropy pass
// does.  0 with *mode, *at (offset in the block) or kBadMsg.
KCDC_ZS_HD int32_t table_place(const uint8_t* blk, uint32_t size, uint32_t t, int16_t* norm, uint32_t* mode,
                               uint32_t* at) {
    LitHdr lh;
    if (lit_header(blk, size, &lh) != 0) return kBadMsg;
    uint32_t pos = lh.hlen + lh.body;
    SeqHdr sh;
    if (seq_header(blk + pos, size - pos, &sh) != 0 || sh.nseq == 0) return kBadMsg;
    pos += sh.hlen;
    static constexpr uint32_t max_log[3] = {kLLLog, kOFLog, kMLLog}, max_sym[3] = {kLLMax, kOFMax, kMLMax};
    for (uint32_t k = 0; k < t; k++) {
        if (seq_mode(sh, k) == 1u) {
            if (size - pos < 1u) return kBadMsg;
            pos += 1u;
        } else if (seq_mode(sh, k) == 2u) {
            uint32_t n = 0, log = 0, used = 0;
            if (fse_read(blk + pos, size - pos, max_log[k], max_sym[k], norm, &n, &log, &used) != 0) return kBadMsg;
            pos += used;
        }
    }
    *mode = seq_mode(sh, t);
    *at = pos;
    return 0;
}

// Builds table t from its description at blk[at..size) under `mode` (not Repeat): 0 with *used the
// description's bytes, or kBadMsg.
KCDC_ZS_HD int32_t table_build(Ctx* c, const uint8_t* blk, uint32_t size, uint32_t at, uint32_t t, uint32_t mode,
                               uint32_t* used) {
    static constexpr uint32_t max_log[3] = {kLLLog, kOFLog, kMLLog}, max_sym[3] = {kLLMax, kOFMax, kMLMax};
    uint32_t* tab = t == 0 ? c->llt : t == 1u ? c->oft : c->mlt;
    uint16_t* next = reinterpret_cast<uint16_t*>(c->w);  // 128 entries; the sequence alphabets have at most 53
    *used = 0;
    if (mode == 1u) {  // RLE: one symbol, no bits
        if (at >= size || blk[at] > max_sym[t]) return kBadMsg;
        tab[0] = blk[at];
        c->log[t] = 0;
        *used = 1;
        return 0;
    }
    uint32_t n = 0, log = 0;
    if (mode == 0) {
        predefined(t, c->norm, &n, &log);
    } else {
        if (at > size || fse_read(blk + at, size - at, max_log[t], max_sym[t], c->norm, &n, &log, used) != 0) return kBadMsg;
    }
    c->log[t] = log;
    return fse_build(c->norm, n, log, tab, next);
}

// Io of the entropy pass: lane() of lanes(), leader(), sync() (the leader's context writes before
// the others' reads), all(st) (a status every lane agrees on: the first non-zero one).
//
// Block bi of a content (a compressed one): its literals into lit_room + its place, its sequences
// into seq_room + its place.  in: the content's bytes; desc: the content's descriptors.
// 0, or kBadMsg.  Room bounds are the index pass's: regen and nseq are read from the descriptor.
template <class Io>
KCDC_ZS_HD int32_t entropy_block(Io& io, Ctx* c, const uint8_t* in, const Desc* desc, uint32_t bi, uint8_t* lit_room,
                                 SeqRec* seq_room) {
    const Desc d = desc[bi];
    const uint8_t* blk = in + dget(d, kFInOff);
    const uint32_t size = static_cast<uint32_t>(dget(d, kFInLen));
    const uint32_t regen = static_cast<uint32_t>(dget(d, kFRegen)), nseq = static_cast<uint32_t>(dget(d, kFNseq));
    uint8_t* lit = lit_room + dget(d, kFLitPos);
    SeqRec* seq = seq_room + dget(d, kFSeqPos);
    if (io.leader()) {  // the literals section's header, the Huffman code, the streams' places
        int32_t st = 0;
        LitHdr lh{};
        c->nstreams = 0;
        if (lit_header(blk, size, &lh) != 0 || lh.regen != regen) st = kBadMsg;
        c->lit_type = lh.type;
        c->seq_at = lh.hlen + lh.body;
        if (st == 0 && lh.type == 1u) c->lit_byte = blk[lh.hlen];
        if (st == 0 && lh.type >= 2u) {
            uint32_t at = lh.hlen, left = lh.comp;  // the streams, after the tree description if there is one
            const uint8_t* tree = blk + lh.hlen;
            uint32_t tree_left = lh.comp;
            if (lh.type == 3u) {  // Treeless: the carrier's description
                const Desc cd = desc[bi - static_cast<uint32_t>(dget(d, kFHufC))];
                const uint8_t* cb = in + dget(cd, kFInOff);
                LitHdr ch{};
                if (lit_header(cb, static_cast<uint32_t>(dget(cd, kFInLen)), &ch) != 0 || ch.type != 2u) st = kBadMsg;
                tree = cb + ch.hlen;
                tree_left = ch.comp;
            }
            uint32_t nsym = 0, used = 0;
            if (st == 0) st = huf_weights(tree, tree_left, c->w, &nsym, &c->huf_bits, &used, c->oft,
                                          reinterpret_cast<uint16_t*>(c->llt), c->norm);
            if (st == 0) {
                huf_build(c->w, nsym, c->huf_bits, c->huf);
                if (lh.type == 2u) {
                    at += used;
                    left -= used;  // used <= comp: huf_weights read inside it
                }
                if (lh.streams == 1u) {
                    c->nstreams = 1;
                    c->s_off[0] = at;
                    c->s_len[0] = left;
                    c->s_out[0] = 0;
                    c->s_cnt[0] = regen;
                } else {
                    const uint32_t seg = (regen + 3u) >> 2;
                    if (left < 6u || 3u * seg > regen) {
                        st = kBadMsg;
                    } else {
                        const uint32_t l1 = le16(blk + at), l2 = le16(blk + at + 2u), l3 = le16(blk + at + 4u);
                        const uint32_t body = left - 6u;
                        if (l1 > body || l2 > body - l1 || l3 > body - l1 - l2) {
                            st = kBadMsg;  // the jump table is larger than its section
                        } else {
                            uint32_t o = at + 6u;
                            c->nstreams = 4;
                            for (uint32_t k = 0; k < 4u; k++) {
                                const uint32_t len = k == 0 ? l1 : k == 1u ? l2 : k == 2u ? l3 : body - l1 - l2 - l3;
                                c->s_off[k] = o;
                                c->s_len[k] = len;
                                c->s_out[k] = k * seg;
                                c->s_cnt[k] = k < 3u ? seg : regen - 3u * seg;
                                o += len;
                            }
                        }
                    }
                }
            }
        }
        c->status = st;
    }
    io.sync();
    int32_t st = c->status;
    if (st != 0) return st;
    if (c->lit_type == 0) {
        const uint8_t* src = blk + (c->seq_at - regen);
        for (uint32_t k = io.lane(); k < regen; k += io.lanes()) lit[k] = src[k];
    } else if (c->lit_type == 1u) {
        const uint8_t v = static_cast<uint8_t>(c->lit_byte);
        for (uint32_t k = io.lane(); k < regen; k += io.lanes()) lit[k] = v;
    } else {  // the streams of a block on separate lanes
        for (uint32_t k = io.lane(); k < c->nstreams; k += io.lanes())
            if (huf_stream(blk + c->s_off[k], c->s_len[k], c->huf, c->huf_bits, lit + c->s_out[k], c->s_cnt[k]) != 0)
                st = kBadMsg;
    }
    st = io.all(st);
    if (st != 0) return st;
    if (io.leader()) {  // the sequences section: tables, then the state walk
        uint32_t pos = c->seq_at;
        SeqHdr sh{};
        if (seq_header(blk + pos, size - pos, &sh) != 0 || sh.nseq != nseq) st = kBadMsg;
        pos += sh.hlen;
        if (st == 0 && nseq != 0) {
            static constexpr Field carrier[3] = {kFLLC, kFOFC, kFMLC};
            for (uint32_t t = 0; t < 3u && st == 0; t++) {
                uint32_t used = 0;
                if (seq_mode(sh, t) != 3u) {
                    st = table_build(c, blk, size, pos, t, seq_mode(sh, t), &used);
                    pos += used;
                } else {  // Repeat_Mode: the carrier's description
                    const Desc cd = desc[bi - static_cast<uint32_t>(dget(d, carrier[t]))];
                    const uint8_t* cb = in + dget(cd, kFInOff);
                    const uint32_t cs = static_cast<uint32_t>(dget(cd, kFInLen));
                    uint32_t mode = 0, at = 0;
                    st = table_place(cb, cs, t, c->norm, &mode, &at);
                    if (st == 0 && mode == 3u) st = kBadMsg;
                    if (st == 0) st = table_build(c, cb, cs, at, t, mode, &used);
                }
            }
            BackBits b;
            if (st == 0 && (pos >= size || !back_init(b, blk + pos, size - pos))) st = kBadMsg;
            if (st == 0) {
                uint32_t ls = back_read(b, c->log[0]), os = back_read(b, c->log[1]), ms = back_read(b, c->log[2]);
                uint32_t lits = 0, total = 0;
                for (uint32_t i = 0; i < nseq; i++) {
                    const uint32_t le = c->llt[ls], oe = c->oft[os], me = c->mlt[ms];
                    const uint32_t oc = fe_sym(oe), mc = fe_sym(me), lc = fe_sym(le);
                    const uint32_t ofv = (1u << oc) + back_read(b, oc);  // oc <= kOFMax = 31
                    const uint32_t ml = ml_base(mc) + back_read(b, ml_bits(mc));
                    const uint32_t ll = ll_base(lc) + back_read(b, ll_bits(lc));
                    if (ll > regen - lits) {  // more literals than the block has
                        st = kBadMsg;
                        break;
                    }
                    lits += ll;
                    if (ll + ml > kBlockMax - total) {  // the block decodes past 128 KiB
                        st = kBadMsg;
                        break;
                    }
                    total += ll + ml;
                    seq[i] = SeqRec{ll, ml, ofv};
                    if (i + 1u < nseq) {
                        ls = fe_base(le) + back_read(b, fe_bits(le));
                        ms = fe_base(me) + back_read(b, fe_bits(me));
                        os = fe_base(oe) + back_read(b, fe_bits(oe));
                    }
                    if (b.pos < 0) {
                        st = kBadMsg;
                        break;
                    }
                }
                if (st == 0 && b.pos != 0) st = kBadMsg;  // not consumed exactly
            }
        }
        c->status = st;
    }
    io.sync();
    return c->status;
}

// ---------------------------------------------------------------- the index pass of one content
// Walks the frames and blocks of in[0..n) and writes their descriptors into desc[0..quota).
// cap: the output slot (clamped to 32 bits by the caller).  0 with *count descriptors, or kBadMsg,
// kOverflow (a header asks for more literal or sequence room than the cap grants, or a
// Frame_Content_Size is over the cap), kNoMem (more blocks than descriptors).
KCDC_ZS_HD int32_t index_content(const uint8_t* in, uint64_t n64, uint32_t header_id, uint32_t cap, Desc* desc,
                                 uint64_t quota, uint32_t* count) {
    *count = 0;
    if (n64 > 0xffffffffull || n64 < 4u) return kBadMsg;  // positions are 32 bits; verifyCompressionHeader
    const uint32_t n = static_cast<uint32_t>(n64);
    const uint32_t id = (uint32_t(in[0]) << 24) | (uint32_t(in[1]) << 16) | (uint32_t(in[2]) << 8) | in[3];
    if (id != header_id) return kBadMsg;
    const uint32_t seq_cap = cap / 3u + 1u;
    uint32_t pos = 4, nd = 0, lit_pos = 0, seq_pos = 0;
    while (pos < n) {  // every round takes at least 4 bytes
        if (n - pos < 4u) return kBadMsg;
        const uint32_t magic = le32(in + pos);
        pos += 4u;
        if ((magic & 0xFFFFFFF0u) == 0x184D2A50u) {  // skippable
            if (n - pos < 4u) return kBadMsg;
            const uint32_t size = le32(in + pos);
            pos += 4u;
            if (size > n - pos) return kBadMsg;
            pos += size;
            continue;
        }
        if (magic != 0xFD2FB528u) return kBadMsg;
        Frame f{};
        if (frame_header(in + pos, n - pos, &f) != 0) return kBadMsg;
        pos += f.hdr_len;
        if (f.has_fcs && f.fcs > cap) return kOverflow;
        if (nd >= quota) return kNoMem;
        const uint32_t fd = nd++;
        const uint32_t window = f.window > 0xffffffffull ? 0xffffffffu : static_cast<uint32_t>(f.window);
        const uint32_t block_max = window < kBlockMax ? window : kBlockMax;
        // carriers: the frame's last Compressed literals, and per table its last non-Repeat mode
        uint32_t huf_at = 0, tab_at[3] = {0, 0, 0};
        bool huf_set = false, tab_set = false;
        for (;;) {  // every round takes at least 3 bytes
            if (n - pos < 3u) return kBadMsg;
            const uint32_t bh = le24(in + pos);
            pos += 3u;
            const uint32_t last = bh & 1u, type = (bh >> 1) & 3u, size = bh >> 3;
            if (type == 3u) return kBadMsg;
            if (size > block_max) return kBadMsg;
            if (nd >= quota) return kNoMem;
            Desc d{};
            dput(d, kFInOff, pos);
            dput(d, kFInLen, size);
            dput(d, kFType, type);
            dput(d, kFLast, last);
            if (type == kTypeRaw) {
                if (size > n - pos) return kBadMsg;
                pos += size;
            } else if (type == kTypeRle) {
                if (n - pos < 1u) return kBadMsg;
                pos += 1u;
            } else {
                if (size > n - pos || size >= kBlockMax || size < 2u) return kBadMsg;
                const uint8_t* blk = in + pos;
                LitHdr lh{};
                if (lit_header(blk, size, &lh) != 0) return kBadMsg;
                const uint32_t sq = lh.hlen + lh.body;
                SeqHdr sh{};
                if (seq_header(blk + sq, size - sq, &sh) != 0) return kBadMsg;
                if (lh.regen > block_max || sh.nseq > (block_max - lh.regen) / 3u) return kBadMsg;  // decodes past the maximum
                if (lh.regen > cap - lit_pos || sh.nseq > seq_cap - seq_pos) return kOverflow;       // ... past the cap
                dput(d, kFRegen, lh.regen);
                dput(d, kFNseq, sh.nseq);
                dput(d, kFLitPos, lit_pos);
                dput(d, kFSeqPos, seq_pos);
                lit_pos += lh.regen;
                seq_pos += sh.nseq;
                if (lh.type == 2u) {
                    huf_at = nd;
                    huf_set = true;
                } else if (lh.type == 3u) {
                    if (!huf_set) return kBadMsg;
                    if (nd - huf_at >= (1u << kCarrierBits)) return kNoMem;
                    dput(d, kFHufC, nd - huf_at);
                }
                if (sh.nseq != 0) {
                    static constexpr Field carrier[3] = {kFLLC, kFOFC, kFMLC};
                    for (uint32_t t = 0; t < 3u; t++) {
                        if (seq_mode(sh, t) != 3u) {
                            tab_at[t] = nd;
                        } else {
                            if (!tab_set) return kBadMsg;
                            if (nd - tab_at[t] >= (1u << kCarrierBits)) return kNoMem;
                            dput(d, carrier[t], nd - tab_at[t]);
                        }
                    }
                    tab_set = true;
                }
                pos += size;
            }
            desc[nd++] = d;
            if (last) break;
        }
        uint32_t sum = 0;
        if (f.checksum) {
            if (n - pos < 4u) return kBadMsg;
            sum = le32(in + pos);
            pos += 4u;
        }
        Desc fr{};
        dput(fr, kFInOff, (f.has_fcs ? kFrameHasSize : 0u) | (f.checksum ? kFrameHasSum : 0u));
        dput(fr, kFType, kTypeFrame);
        fr.q[1] = (f.fcs & 0xffffffffull) | (uint64_t(sum) << 32);
        fr.q[2] = window;
        desc[fd] = fr;
    }
    *count = nd;
    return 0;
}

// ---------------------------------------------------------------- the execute pass of one content
// RFC 8878 3.1.1.5: the offset of a sequence and the history after it.  false: offset 0.
KCDC_ZS_HD bool resolve_offset(uint32_t ofv, uint32_t ll, uint32_t* rep, uint32_t* off) {
    if (ofv > 3u) {
        *off = ofv - 3u;
        rep[2] = rep[1];
        rep[1] = rep[0];
        rep[0] = *off;
        return true;
    }
    const uint32_t idx = ofv - 1u + (ll == 0 ? 1u : 0u);  // 0..3
    if (idx == 0) {
        *off = rep[0];
        return true;
    }
    const uint32_t o = idx == 3u ? rep[0] - 1u : rep[idx];
    if (o == 0) return false;
    if (idx != 1u) rep[2] = rep[1];
    rep[1] = rep[0];
    rep[0] = o;
    *off = o;
    return true;
}

// The plan of one batch: where each sequence's literals come from and go to, and its match.
struct Plan {
    uint32_t at[kZstdBatch + 1];  // first output byte of sequence j (its literals); [cnt]: the batch's end
    uint32_t lit[kZstdBatch], ll[kZstdBatch], ml[kZstdBatch], off[kZstdBatch];
    int32_t status;
    uint32_t lit_used;  // literals of the block used after this batch
    uint32_t rep[3];
    uint32_t trail;
};

// Whether sequence j's match reads only bytes before `first`, the batch's first output byte
// (off <= its place in the frame: the plan's check, so src does not wrap).
KCDC_ZS_HD bool match_early(const Plan* p, uint32_t j, uint32_t first) {
    const uint32_t src = p->at[j] + p->ll[j] - p->off[j];
    return src <= first && p->ml[j] <= first - src;
}

// Io of the execute pass: lane(), lanes(), leader(), sync(), fence() (this wave's output stores
// before its later output loads), copy(dst, src, len), fill(dst, byte, len), match(dst, len, dist).
//
// The content's blocks in order into out[0..cap).  p: the plan room.  0 with *total the decoded
// length, kBadMsg or kOverflow.  The leader plans (every bound is decided there); all lanes copy.
template <class Io>
KCDC_ZS_HD int32_t execute_content(Io& io, Plan* p, const uint8_t* in, Desc* desc, uint32_t ndesc,
                                   const uint8_t* lit_room, const SeqRec* seq_room, uint8_t* out, uint32_t cap,
                                   uint32_t* total) {
    uint32_t o = 0, frame_at = 0, frame_desc = 0, window = 0, flags = 0, fcs = 0;
    if (io.leader()) {
        p->rep[0] = 1;
        p->rep[1] = 4;
        p->rep[2] = 8;
    }
    for (uint32_t bi = 0; bi < ndesc; bi++) {
        const Desc d = desc[bi];
        const uint32_t type = static_cast<uint32_t>(dget(d, kFType));
        const uint32_t size = static_cast<uint32_t>(dget(d, kFInLen));
        const uint8_t* blk = in + dget(d, kFInOff);
        if (type == kTypeFrame) {
            frame_at = o;
            frame_desc = bi;
            flags = static_cast<uint32_t>(dget(d, kFInOff));
            fcs = static_cast<uint32_t>(d.q[1]);
            window = static_cast<uint32_t>(d.q[2]);
            io.sync();
            if (io.leader()) {
                p->rep[0] = 1;
                p->rep[1] = 4;
                p->rep[2] = 8;
            }
            io.sync();
            continue;
        }
        const uint32_t block_at = o;
        const uint32_t block_max = window < kBlockMax ? window : kBlockMax;
        if (type == kTypeRaw) {
            if (size > cap - o) return kOverflow;
            io.copy(out + o, blk, size);
            o += size;
        } else if (type == kTypeRle) {
            if (size > cap - o) return kOverflow;
            io.fill(out + o, blk[0], size);
            o += size;
        } else {
            const uint32_t regen = static_cast<uint32_t>(dget(d, kFRegen)), nseq = static_cast<uint32_t>(dget(d, kFNseq));
            const uint8_t* lit = lit_room + dget(d, kFLitPos);
            const SeqRec* seq = seq_room + dget(d, kFSeqPos);
            uint32_t lit_used = 0;
            for (uint32_t base = 0; base < nseq; base += kZstdBatch) {
                const uint32_t cnt = nseq - base < kZstdBatch ? nseq - base : kZstdBatch;
                io.sync();  // the previous plan's readers are done
                for (uint32_t j = io.lane(); j < cnt; j += io.lanes()) {  // the batch's records, one load a lane
                    const SeqRec r = seq[base + j];
                    p->ll[j] = r.ll;
                    p->ml[j] = r.ml;
                    p->off[j] = r.ofv;
                }
                io.sync();
                if (io.leader()) {  // 1, 2: the repeat offsets, the positions, every bound
                    int32_t st = 0;
                    uint32_t at = o, lu = lit_used;
                    for (uint32_t j = 0; j < cnt; j++) {
                        const SeqRec r{p->ll[j], p->ml[j], p->off[j]};
                        uint32_t off = 0;
                        if (r.ll > regen - lu || !resolve_offset(r.ofv, r.ll, p->rep, &off)) {
                            st = kBadMsg;
                            break;
                        }
                        if (r.ll > cap - at || r.ml > cap - at - r.ll) {
                            st = kOverflow;
                            break;
                        }
                        if (r.ll + r.ml > block_max - (at - block_at)) {  // the block decodes past its maximum
                            st = kBadMsg;
                            break;
                        }
                        // beyond what the frame has produced, or beyond the window
                        if (off > at + r.ll - frame_at || off > window) {
                            st = kBadMsg;
                            break;
                        }
                        p->at[j] = at;
                        p->lit[j] = lu;
                        p->off[j] = off;
                        at += r.ll + r.ml;
                        lu += r.ll;
                    }
                    p->at[cnt] = at;
                    p->lit_used = lu;
                    p->status = st;
                }
                io.sync();
                if (p->status != 0) return p->status;
                const uint32_t first = o, nbytes = p->at[cnt] - o;
                io.fence();
                // 3, 4: lanes over the batch's output bytes: every literal, and every match whose
                // source ends at or before the batch's first byte
                for (uint32_t k = io.lane(); k < nbytes; k += io.lanes()) {
                    uint32_t lo = 0, hi = cnt;  // the sequence holding byte k: at[lo] <= first + k < at[lo + 1]
                    while (hi - lo > 1u) {
                        const uint32_t mid = (lo + hi) >> 1;
                        if (p->at[mid] - first <= k) lo = mid; else hi = mid;
                    }
                    const uint32_t r = first + k - p->at[lo];
                    if (r < p->ll[lo]) {
                        out[first + k] = lit[p->lit[lo] + r];
                    } else if (match_early(p, lo, first)) {
                        out[first + k] = out[p->at[lo] + p->ll[lo] - p->off[lo] + (r - p->ll[lo])];
                    }
                }
                io.fence();  // 5
                // 6: the other matches in order
                for (uint32_t j = 0; j < cnt; j++) {
                    if (match_early(p, j, first)) continue;
                    const uint32_t ms = p->at[j] + p->ll[j];
                    io.match(out + ms, p->ml[j], p->off[j]);
                    io.fence();
                }
                o = p->at[cnt];
                lit_used = p->lit_used;
            }
            const uint32_t trail = regen - lit_used;  // lit_used <= regen: the plan's first check
            if (trail > cap - o) return kOverflow;
            if (trail > block_max - (o - block_at)) return kBadMsg;
            io.copy(out + o, lit + lit_used, trail);
            o += trail;
        }
        if (o - block_at > block_max) return kBadMsg;
        if (dget(d, kFLast)) {
            if ((flags & kFrameHasSize) && fcs != o - frame_at) return kBadMsg;
            if (io.leader()) {
                desc[frame_desc].q[2] = window | (uint64_t(frame_at) << 32);
                desc[frame_desc].q[3] = o - frame_at;
            }
        }
    }
    *total = o;
    return 0;
}

// ---------------------------------------------------------------- XXH64 (seed 0)
constexpr uint64_t kP1 = 0x9E3779B185EBCA87ull, kP2 = 0xC2B2AE3D27D4EB4Full, kP3 = 0x165667B19E3779F9ull,
                   kP4 = 0x85EBCA77C2B2AE63ull, kP5 = 0x27D4EB2F165667C5ull;
KCDC_ZS_HD uint64_t rotl64(uint64_t v, uint32_t r) { return (v << r) | (v >> (64u - r)); }
KCDC_ZS_HD uint64_t xxh_round(uint64_t acc, uint64_t v) { return rotl64(acc + v * kP2, 31) * kP1; }
KCDC_ZS_HD uint64_t xxh_merge(uint64_t h, uint64_t v) { return (h ^ xxh_round(0, v)) * kP1 + kP4; }
KCDC_ZS_HD uint64_t xxh_init(uint32_t lane) {  // accumulator `lane` of the four
    return lane == 0 ? kP1 + kP2 : lane == 1u ? kP2 : lane == 2u ? 0u : 0u - kP1;
}
// The hash of `len` bytes whose stripes gave v[0..4) (len >= 32) and whose last len % 32 bytes are at tail.
KCDC_ZS_HD uint64_t xxh_finish(const uint64_t* v, const uint8_t* tail, uint64_t len) {
    uint64_t h;
    if (len >= 32u) {
        h = rotl64(v[0], 1) + rotl64(v[1], 7) + rotl64(v[2], 12) + rotl64(v[3], 18);
        for (uint32_t k = 0; k < 4u; k++) h = xxh_merge(h, v[k]);
    } else {
        h = kP5;
    }
    h += len;
    uint32_t left = static_cast<uint32_t>(len & 31u);
    for (; left >= 8u; left -= 8u, tail += 8) h = rotl64(h ^ xxh_round(0, le64(tail)), 27) * kP1 + kP4;
    if (left >= 4u) {
        h = rotl64(h ^ (uint64_t(le32(tail)) * kP1), 23) * kP2 + kP3;
        tail += 4;
        left -= 4u;
    }
    for (; left; left--, tail++) h = rotl64(h ^ (uint64_t(*tail) * kP5), 11) * kP1;
    h ^= h >> 33;
    h *= kP2;
    h ^= h >> 29;
    h *= kP3;
    h ^= h >> 32;
    return h;
}
KCDC_ZS_HD uint64_t xxh64(const uint8_t* p, uint64_t len) {
    uint64_t v[4] = {xxh_init(0), xxh_init(1), xxh_init(2), xxh_init(3)};
    const uint64_t stripes = len >> 5;
    for (uint64_t s = 0; s < stripes; s++)
        for (uint32_t k = 0; k < 4u; k++) v[k] = xxh_round(v[k], le64(p + 32u * s + 8u * k));
    return xxh_finish(v, p + 32u * stripes, len);
}

}  // namespace zsf
}  // namespace kcdc
