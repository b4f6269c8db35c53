// Every decision the inflate decoder takes on untrusted bytes, for the device kernels
// (kcdc_inflate.hip) and the host program that runs the tests' vectors under the sanitizers
// (tools/inflate_host.cpp): the header ID, the RFC 1952 member header walk and trailer, RFC 1951
// block headers, the dynamic header with its code-length checks, the decode tables, the length and
// distance base / extra-bit tables, and every bound on input, output and table room.  What the
// reference's readers accept (compressor_deflate.go:64-78: klauspost/compress/flate.NewReader;
// compressor_gzip.go:68-85: compress/gzip.NewReader; compressor_pgzip.go: pgzip.NewReader).
//
// The decoder is written once, over an `Io` that supplies the bytes, the bit buffer, the table
// memory and the three ways of producing output (a literal, a match, a stored run).  The host Io
// is sequential over exactly-sized heap buffers; the device Io is one wave (every call is
// wave-uniform).  All lengths are compared against what is left and never added first.
//
// Where readers differ, this follows Go's:
//  * bytes after the final block of a raw stream are ignored (flate's reader stops at the final
//    block and compressor_deflate.go:64-78 reads nothing further).  oracle/deflate.py::decompress
//    refuses them (zlib's unused_data must be empty): the oracle is stricter here;
//  * a code with a single one-bit length is the only incomplete code accepted, for the
//    literal/length, distance and code-length codes alike (huffmanDecoder.init: `code != 1<<max &&
//    !(code == 1 && max == 1)`); zlib accepts it for the first two only;
//  * a literal/length code with no length for symbol 256 is not refused at the header
//    (flate's readHuffman only uses that length as a lower bound of the bits to read; zlib's
//    inflate answers "missing end-of-block"): such a block can only end in truncation or an error;
//  * reserved FLG bits of a member header are ignored (gzip's readHeader tests FEXTRA, FNAME,
//    FCOMMENT and FHCRC only; zlib answers "unknown header flags set");
//  * FNAME and FCOMMENT are limited to 511 bytes and their NUL (readString's 512-byte buffer).
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define KCDC_INF_HD __host__ __device__ inline
#else
#define KCDC_INF_HD inline
#endif

namespace kcdc {
namespace inff {

constexpr int32_t kBadMsg = -74, kOverflow = -75;  // KCDC_EBADMSG, KCDC_EOVERFLOW

constexpr uint32_t kMaxLit = 286, kMaxDist = 30, kMaxLens = 320;  // 288 + 32 lengths of a dynamic header
constexpr uint32_t kLitRoot = 9, kDistRoot = 6, kClRoot = 7;
// zlib's proven table bounds (inftrees.h ENOUGH_LENS, ENOUGH_DISTS) for these root bits
constexpr uint32_t kLitCap = 852, kDistCap = 592;
constexpr uint32_t kFixLitCap = 512, kFixDistCap = 64;  // the fixed code: 9-bit and 5-bit codes in root tables

// A table entry: bits 0..7 the code bits to drop, 8..15 the operation, 16..31 a value.
constexpr uint32_t kOpLit = 0x00;    // value: the byte
constexpr uint32_t kOpBase = 0x10;   // | extra bits (0..13); value: the length or distance base
constexpr uint32_t kOpEnd = 0x20;    // end of block
constexpr uint32_t kOpBad = 0x40;    // no code, or a symbol that may not be used
constexpr uint32_t kOpLink = 0x80;   // | index bits of a sub-table; value: its offset
KCDC_INF_HD uint32_t entry(uint32_t bits, uint32_t op, uint32_t val) { return bits | (op << 8) | (val << 16); }
KCDC_INF_HD uint32_t e_bits(uint32_t e) { return e & 255u; }
KCDC_INF_HD uint32_t e_op(uint32_t e) { return (e >> 8) & 255u; }
KCDC_INF_HD uint32_t e_val(uint32_t e) { return e >> 16; }

constexpr int kCodeLit = 0, kCodeDist = 1, kCodeCl = 2;

// The entry of symbol `sym` of a code of the given kind, without its code bits.
KCDC_INF_HD uint32_t symbol_entry(int kind, uint32_t sym) {
    // RFC 1951 3.2.5
    constexpr uint16_t len_base[29] = {3,  4,  5,  6,  7,  8,  9,  10, 11,  13,  15,  17,  19,  23, 27,
                                       31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
    constexpr uint8_t len_extra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
    constexpr uint16_t dist_base[30] = {1,   2,   3,   4,   5,   7,    9,    13,   17,   25,   33,   49,   65,    97,    129,
                                        193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
    constexpr uint8_t dist_extra[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
    if (kind == kCodeCl) return entry(0, kOpLit, sym);
    if (kind == kCodeDist) return sym < 30u ? entry(0, kOpBase | dist_extra[sym], dist_base[sym]) : entry(0, kOpBad, 0);
    if (sym < 256u) return entry(0, kOpLit, sym);
    if (sym == 256u) return entry(0, kOpEnd, 0);
    return sym < 286u ? entry(0, kOpBase | len_extra[sym - 257u], len_base[sym - 257u]) : entry(0, kOpBad, 0);
}

// Scratch of one table build, in the Io's memory.
struct Build {
    uint16_t count[16];   // codes of each length
    uint16_t offs[16];    // first place of each length in `work`
    uint16_t work[kMaxLens];  // symbols in code order
};

// The decode table of the code lens[0..n) (each 0..15), root index bits, at most cap entries:
// zlib's inflate_table with a root that is never adjusted (the table is invalid-filled first, so
// shorter and incomplete codes leave refusing entries).  0, or kBadMsg for an over-subscribed code,
// an incomplete code other than a single one-bit code, or a table beyond cap (no valid code).
template <class Io>
KCDC_INF_HD int32_t build_table(Io& io, const uint8_t* lens, uint32_t n, int kind, uint32_t root, uint32_t* tab,
                                uint32_t cap, Build* b) {
    for (uint32_t k = 0; k < 16u; k++) b->count[k] = 0;
    for (uint32_t s = 0; s < n; s++) b->count[lens[s]]++;
    io.fill(tab, 0, 1, 1u << root, entry(1, kOpBad, 0));
    uint32_t max = 15;
    while (max >= 1u && b->count[max] == 0) max--;
    if (max == 0) return 0;  // no code at all: every lookup refuses (Go: "fails later if the tree is used")
    uint32_t min = 1;
    while (b->count[min] == 0) min++;
    int32_t left = 1;
    for (uint32_t k = 1; k <= 15u; k++) {
        left <<= 1;
        left -= static_cast<int32_t>(b->count[k]);
        if (left < 0) return kBadMsg;  // over-subscribed
    }
    if (left > 0 && !(max == 1u && b->count[1] == 1u)) return kBadMsg;  // incomplete
    b->offs[1] = 0;
    for (uint32_t k = 1; k < 15u; k++) b->offs[k + 1] = static_cast<uint16_t>(b->offs[k] + b->count[k]);
    for (uint32_t s = 0; s < n; s++)
        if (lens[s]) b->work[b->offs[lens[s]]++] = static_cast<uint16_t>(s);
    const uint32_t mask = (1u << root) - 1u;
    uint32_t huff = 0, sym = 0, len = min, next = 0, curr = root, drop = 0, low = ~0u, used = 1u << root;
    if (used > cap) return kBadMsg;
    for (;;) {
        if (len > root && (huff & mask) != low) {  // a new sub-table
            if (drop == 0) drop = root;
            next += 1u << curr;
            curr = len - drop;
            int32_t room = 1 << curr;
            while (curr + drop < max) {
                room -= static_cast<int32_t>(b->count[curr + drop]);
                if (room <= 0) break;
                curr++;
                room <<= 1;
            }
            if ((1u << curr) > cap - used) return kBadMsg;
            used += 1u << curr;
            low = huff & mask;
            io.fill(tab, low, 1, low + 1u, entry(root, kOpLink | curr, next));
        }
        const uint32_t here = symbol_entry(kind, b->work[sym]) | (len - drop);
        io.fill(tab + next, huff >> drop, 1u << (len - drop), 1u << curr, here);
        uint32_t incr = 1u << (len - 1u);  // backwards increment of the len-bit code
        while (huff & incr) incr >>= 1;
        huff = incr ? (huff & (incr - 1u)) + incr : 0u;
        sym++;
        if (--b->count[len] == 0) {
            if (len == max) break;
            len = lens[b->work[sym]];
        }
    }
    return 0;
}

// The bit buffer: a 64-bit window of the stream, refilled by the Io.  After io.refill(bb) it holds
// at least 33 bits or every remaining bit of the content; bits above `cnt` are zero.  P is the
// Io's pos_t, the type of positions in the content and in the output: uint64_t on the host; the
// device takes uint32_t (positions live in SGPRs there) and refuses contents of 4 GiB or more.
template <class P>
struct Bits {
    uint64_t buf;
    uint32_t cnt;
    P pos;  // the next content byte to enter the buffer
};
template <class B>
KCDC_INF_HD uint32_t peek(const B& bb, uint32_t n) { return static_cast<uint32_t>(bb.buf) & ((1u << n) - 1u); }
template <class B>
KCDC_INF_HD void drop_bits(B& bb, uint32_t n) {
    bb.buf >>= n;
    bb.cnt -= n;
}
// n <= 16 bits into *v, or false when the content ends first.
template <class B>
KCDC_INF_HD bool take(B& bb, uint32_t n, uint32_t* v) {
    if (n > bb.cnt) return false;
    *v = peek(bb, n);
    drop_bits(bb, n);
    return true;
}

// One symbol through a two-level table.  False: the content ends inside the code.  io.u(v) is v
// (the device says with it that v is the same in every lane).
template <class Io, class B>
KCDC_INF_HD bool lookup(Io& io, B& bb, const uint32_t* tab, uint32_t root, uint32_t* e) {
    uint32_t h = io.u(tab[peek(bb, root)]);
    if (e_op(h) & kOpLink) {
        const uint32_t sub = e_op(h) & 15u;
        h = io.u(tab[e_val(h) + (peek(bb, root + sub) >> root)]);
        if (root + e_bits(h) > bb.cnt) return false;
        drop_bits(bb, root + e_bits(h));
    } else {
        if (e_bits(h) > bb.cnt) return false;
        drop_bits(bb, e_bits(h));
    }
    *e = h;
    return true;
}

// The literal whose code starts at the low bit of `bits` (15 bits of the stream), as its code
// bits | byte << 8, or 0 if the code there is not a literal's.
KCDC_INF_HD uint32_t literal_at(const uint32_t* tab, uint32_t bits) {
    uint32_t h = tab[bits & ((1u << kLitRoot) - 1u)], n = 0;
    if (e_op(h) & kOpLink) {
        n = kLitRoot;
        h = tab[e_val(h) + ((bits >> kLitRoot) & ((1u << (e_op(h) & 15u)) - 1u))];
    }
    return e_op(h) == kOpLit ? (n + e_bits(h)) | (e_val(h) << 8) : 0u;
}

// A run of literals ahead of the symbol loop.  io.top_up(bb) fills the buffer to 57 bits or more (or
// with all that is left); io.look_ahead(bb, tab, held) looks up literal_at for each of the `held`
// bit positions whose 15 bits the buffer holds (the device: lane k takes position k, one LDS access
// for all of them) and io.looked(c, at) reads position at's back.  The walk goes from literal to
// literal until it meets another kind of symbol (or no code), the cap, or a position past `held`:
// what the symbol loop decides for each literal, taken one LDS round trip for several.
template <class Io, class B>
KCDC_INF_HD void literal_run(Io& io, B& bb, const uint32_t* tab, typename Io::pos_t cap, typename Io::pos_t* o) {
    for (;;) {
        io.top_up(bb);
        if (bb.cnt < 15u) return;
        const uint32_t held = bb.cnt - 14u;  // <= 50
        const auto c = io.look_ahead(bb, tab, held);
        uint32_t at = 0;
        while (at < held && *o < cap) {
            const uint32_t e = io.looked(c, at);
            if (e == 0) break;
            io.literal(*o, e >> 8);
            *o += 1;
            at += e & 255u;  // the literal started below held, so it ends inside the buffer
        }
        if (at == 0) return;
        drop_bits(bb, at);
        if (at < held) return;  // stopped at a symbol of another kind, or at the cap
    }
}

// The tables of the fixed code (RFC 1951 3.2.6) into flt[kFixLitCap], fdt[kFixDistCap].
template <class Io>
KCDC_INF_HD void build_fixed(Io& io, uint8_t* lens, uint32_t* flt, uint32_t* fdt, Build* b) {
    for (uint32_t s = 0; s < 288u; s++) lens[s] = s < 144u ? 8 : s < 256u ? 9 : s < 280u ? 7 : 8;
    (void)build_table(io, lens, 288, kCodeLit, kLitRoot, flt, kFixLitCap, b);
    for (uint32_t s = 0; s < 32u; s++) lens[s] = 5;
    (void)build_table(io, lens, 32, kCodeDist, kDistRoot, fdt, kFixDistCap, b);
}

// The header of a dynamic block (RFC 1951 3.2.7) from the bit buffer into the Io's tables.
template <class Io, class B>
KCDC_INF_HD int32_t dynamic_header(Io& io, B& bb) {
    uint32_t v = 0;
    io.refill(bb);
    if (!take(bb, 14, &v)) return kBadMsg;
    const uint32_t nlit = 257u + (v & 31u), ndist = 1u + ((v >> 5) & 31u), ncl = 4u + (v >> 10);
    if (nlit > kMaxLit || ndist > kMaxDist) return kBadMsg;
    constexpr uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    uint8_t* lens = io.lens();
    for (uint32_t k = 0; k < 19u; k++) lens[k] = 0;
    for (uint32_t k = 0; k < ncl; k++) {
        io.refill(bb);
        if (!take(bb, 3, &v)) return kBadMsg;
        lens[order[k]] = static_cast<uint8_t>(v);
    }
    uint32_t* cl = io.dist_table();  // the code-length code's table lives where the distance table will
    if (build_table(io, lens, 19, kCodeCl, kClRoot, cl, 1u << kClRoot, io.build()) != 0) return kBadMsg;
    const uint32_t total = nlit + ndist;
    uint32_t i = 0, prev = 0;
    while (i < total) {
        io.refill(bb);
        uint32_t e = 0;
        if (!lookup(io, bb, cl, kClRoot, &e)) return kBadMsg;
        if (e_op(e) != kOpLit) return kBadMsg;
        const uint32_t s = e_val(e);
        if (s < 16u) {
            lens[i++] = static_cast<uint8_t>(s);
            prev = s;
            continue;
        }
        uint32_t rep = 0, val = 0;
        if (s == 16u) {
            if (i == 0) return kBadMsg;  // nothing to repeat
            if (!take(bb, 2, &v)) return kBadMsg;
            rep = 3u + v;
            val = prev;
        } else if (s == 17u) {
            if (!take(bb, 3, &v)) return kBadMsg;
            rep = 3u + v;
        } else {
            if (!take(bb, 7, &v)) return kBadMsg;
            rep = 11u + v;
        }
        if (rep > total - i) return kBadMsg;  // the run leaves the lengths
        for (uint32_t k = 0; k < rep; k++) lens[i + k] = static_cast<uint8_t>(val);
        i += rep;
        prev = val;
    }
    if (build_table(io, lens, nlit, kCodeLit, kLitRoot, io.lit_table(), kLitCap, io.build()) != 0) return kBadMsg;
    if (build_table(io, lens + nlit, ndist, kCodeDist, kDistRoot, io.dist_table(), kDistCap, io.build()) != 0)
        return kBadMsg;
    return 0;
}

// One raw RFC 1951 stream from content byte `start` on: output from *o (<= cap) on, distances
// reaching back to the stream's own first output byte (*o at the call).  0 with *end the byte after
// the final block, kBadMsg, kOverflow.
template <class Io>
KCDC_INF_HD int32_t inflate_raw(Io& io, typename Io::pos_t start, typename Io::pos_t cap, typename Io::pos_t* o,
                                typename Io::pos_t* end) {
    typedef typename Io::pos_t P;
    const P origin = *o;
    Bits<P> bb{0, 0, start};
    uint32_t v = 0;
    for (;;) {
        io.refill(bb);
        if (!take(bb, 3, &v)) return kBadMsg;
        const uint32_t final_block = v & 1u, type = v >> 1;
        if (type == 3u) return kBadMsg;
        if (type == 0u) {
            drop_bits(bb, bb.cnt & 7u);
            io.refill(bb);
            uint32_t len = 0, nlen = 0;
            if (!take(bb, 16, &len) || !take(bb, 16, &nlen)) return kBadMsg;
            if ((len ^ nlen) != 0xffffu) return kBadMsg;
            const P at = bb.pos - (bb.cnt >> 3);  // whole bytes in the buffer go back to the input
            bb.buf = 0;
            bb.cnt = 0;
            if (len > io.size() - at) return kBadMsg;
            if (len > cap - *o) return kOverflow;
            io.stored(at, *o, len);
            bb.pos = at + len;
            *o += len;
        } else {
            const uint32_t *lt = io.fixed_lit_table(), *dt = io.fixed_dist_table();
            if (type == 2u) {
                const int32_t st = dynamic_header(io, bb);
                if (st != 0) return st;
                lt = io.lit_table();
                dt = io.dist_table();
            }
            uint32_t run = 0;  // literals in a row
            for (;;) {
                // after two literals more are likely: take them ahead of the loop (a look-ahead
                // that meets a match at once is a lookup wasted, so not before)
                if (run >= 2u) literal_run(io, bb, lt, cap, o);
                io.refill(bb);
                uint32_t e = 0;
                if (!lookup(io, bb, lt, kLitRoot, &e)) return kBadMsg;
                const uint32_t op = e_op(e);
                if (op == kOpLit) {
                    if (*o >= cap) return kOverflow;
                    io.literal(*o, e_val(e));
                    *o += 1;
                    run++;
                    continue;
                }
                run = 0;
                if (op == kOpEnd) break;
                if (!(op & kOpBase)) return kBadMsg;  // no such code, or symbol 286 / 287
                if (!take(bb, op & 15u, &v)) return kBadMsg;
                const uint32_t len = e_val(e) + v;
                io.refill(bb);
                if (!lookup(io, bb, dt, kDistRoot, &e)) return kBadMsg;
                if (!(e_op(e) & kOpBase)) return kBadMsg;  // no such code, or symbol 30 / 31
                if (!take(bb, e_op(e) & 15u, &v)) return kBadMsg;
                const uint32_t dist = e_val(e) + v;
                if (dist > *o - origin) return kBadMsg;  // before the stream's first output byte
                if (len > cap - *o) return kOverflow;
                io.match(*o, len, dist);
                *o += len;
            }
        }
        if (final_block) break;
    }
    *end = bb.pos - (bb.cnt >> 3);
    return 0;
}

KCDC_INF_HD uint32_t crc32_byte(uint32_t c, uint32_t b) {
    c ^= b;
    for (int k = 0; k < 8; k++) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u)));
    return c;
}

// The member header at content byte *pos (RFC 1952 2.3; gzip.Reader.readHeader): 0 with *pos the
// first byte of the stream, or kBadMsg.
template <class Io>
KCDC_INF_HD int32_t gzip_header(Io& io, typename Io::pos_t* pos) {
    const typename Io::pos_t n = io.size();
    typename Io::pos_t i = *pos;
    uint32_t crc = 0xffffffffu;
    auto next = [&](uint32_t* b) -> bool {
        if (i >= n) return false;
        *b = io.byte(i++);
        crc = crc32_byte(crc, *b);
        return true;
    };
    uint32_t b = 0, b2 = 0, magic = 0, flg = 0;
    for (uint32_t k = 0; k < 3u; k++) {
        if (!next(&b)) return kBadMsg;
        magic |= b << (8u * k);
    }
    if (magic != 0x088b1fu) return kBadMsg;  // ID1, ID2, CM = 8
    if (!next(&flg)) return kBadMsg;
    for (uint32_t k = 0; k < 6u; k++)  // MTIME, XFL, OS
        if (!next(&b)) return kBadMsg;
    if (flg & 4u) {  // FEXTRA
        if (!next(&b) || !next(&b2)) return kBadMsg;
        for (uint32_t left = b | (b2 << 8); left; left--)
            if (!next(&b)) return kBadMsg;
    }
    for (uint32_t f = 8u; f <= 16u; f <<= 1) {  // FNAME, FCOMMENT
        if (!(flg & f)) continue;
        for (uint32_t k = 0;; k++) {
            if (k >= 512u || !next(&b)) return kBadMsg;
            if (b == 0) break;
        }
    }
    if (flg & 2u) {  // FHCRC: the low 16 bits of the CRC-32 of the header so far
        const uint32_t want = (crc ^ 0xffffffffu) & 0xffffu;
        if (!next(&b) || !next(&b2)) return kBadMsg;
        if ((b | (b2 << 8)) != want) return kBadMsg;
    }
    *pos = i;
    return 0;
}

// A content = BE32(header ID) || stream.  gz: RFC 1952 members (one or more, their output
// appended), each with its CRC-32 and ISIZE checked; else one raw stream, whatever follows it
// ignored.  The first member's CRC is handed to io.first_member (the device checks it in a pass of
// its own), a later member's to io.member_crc, which answers at once.
// 0 with *total the decoded length, kBadMsg or kOverflow.
template <class Io>
KCDC_INF_HD int32_t inflate_content(Io& io, uint32_t header_id, bool gz, typename Io::pos_t cap,
                                    typename Io::pos_t* total) {
    typedef typename Io::pos_t P;
    *total = 0;
    const P n = io.size();
    if (n < 4u) return kBadMsg;  // verifyCompressionHeader
    const uint32_t id = (io.byte(0) << 24) | (io.byte(1) << 16) | (io.byte(2) << 8) | io.byte(3);
    if (id != header_id) return kBadMsg;
    P o = 0, pos = 4;
    if (!gz) {
        const int32_t st = inflate_raw(io, pos, cap, &o, &pos);
        if (st == 0) *total = o;
        return st;
    }
    for (uint32_t member = 0;; member++) {
        int32_t st = gzip_header(io, &pos);
        if (st != 0) return st;
        const P from = o;
        st = inflate_raw(io, pos, cap, &o, &pos);
        if (st != 0) return st;
        if (n - pos < 8u) return kBadMsg;  // pos <= n
        uint32_t crc = 0, isize = 0;
        for (uint32_t k = 0; k < 4u; k++) {
            crc |= io.byte(pos + k) << (8u * k);
            isize |= io.byte(pos + 4u + k) << (8u * k);
        }
        if (isize != static_cast<uint32_t>(o - from)) return kBadMsg;
        if (member == 0)
            io.first_member(o, crc);
        else if (!io.member_crc(from, o - from, crc))
            return kBadMsg;
        pos += 8;
        if (pos == n) break;  // a clean end; anything else must be another whole member
    }
    *total = o;
    return 0;
}

}  // namespace inff
}  // namespace kcdc
