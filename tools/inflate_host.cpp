// The inflate decoder's decisions on the CPU, under the host sanitizers: decodes the vector files
// that tests/inflate_vectors.py writes through kopia_amd/csrc/kcdc_inflate_format.h, the header the
// device kernels decide with, sequentially, with the content, the output slot and every table in
// heap buffers of exactly their size, so a read or write outside any of them is a sanitizer
// report.  Every valid and corrupt vector runs here before it is sent to a GPU.
//   make build/inflate_host      (g++ -fsanitize=address,undefined -fno-sanitize-recover=all)
//   build/inflate_host vectors.bin
// File (little-endian): "INFVEC1\0", u32 count, then per vector: u32 header ID, u32 gzip member
// framing (0 / 1), u64 cap, i32 expected status, u64 n, n content bytes, u64 m, m expected bytes.
// Prints one line per vector; exit status 1 if any status or byte differs from the expectation.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "kcdc_inflate_format.h"

using namespace kcdc;

namespace {

template <typename T>
T* exact(size_t count) { return static_cast<T*>(malloc(count * sizeof(T))); }  // 0: a zero-size block, any access is a report

uint32_t crc32(const uint8_t* p, uint64_t n) {
    uint32_t c = 0xFFFFFFFFu;
    for (uint64_t i = 0; i < n; i++) c = inff::crc32_byte(c, p[i]);
    return c ^ 0xFFFFFFFFu;
}

// The sequential Io: what the device's wave does, one byte at a time.
struct HostIo {
    typedef uint64_t pos_t;
    const uint8_t* in;
    uint64_t n;
    uint8_t* out;
    uint32_t *lt, *dt, *flt, *fdt;
    uint8_t* len_room;
    inff::Build* b;
    uint64_t first_len = 0;
    uint32_t first_crc = 0;
    bool gz_seen = false;

    HostIo(const uint8_t* in_, uint64_t n_, uint8_t* out_) : in(in_), n(n_), out(out_) {
        lt = exact<uint32_t>(inff::kLitCap);
        dt = exact<uint32_t>(inff::kDistCap);
        flt = exact<uint32_t>(inff::kFixLitCap);
        fdt = exact<uint32_t>(inff::kFixDistCap);
        len_room = exact<uint8_t>(inff::kMaxLens);
        b = exact<inff::Build>(1);
        inff::build_fixed(*this, len_room, flt, fdt, b);
    }
    ~HostIo() {
        free(lt);
        free(dt);
        free(flt);
        free(fdt);
        free(len_room);
        free(b);
    }
    uint64_t size() const { return n; }
    uint32_t byte(uint64_t i) const { return in[i]; }
    uint32_t u(uint32_t v) const { return v; }
    void refill(inff::Bits<pos_t>& bb) const {
        while (bb.cnt <= 56u && bb.pos < n) {
            bb.buf |= uint64_t(in[bb.pos++]) << bb.cnt;
            bb.cnt += 8;
        }
    }
    void fill(uint32_t* tab, uint32_t start, uint32_t step, uint32_t end, uint32_t val) const {
        for (uint32_t i = start; i < end; i += step) tab[i] = val;
    }
    uint8_t* lens() { return len_room; }
    inff::Build* build() { return b; }
    uint32_t* lit_table() { return lt; }
    uint32_t* dist_table() { return dt; }
    const uint32_t* fixed_lit_table() const { return flt; }
    const uint32_t* fixed_dist_table() const { return fdt; }
    // inff::literal_run's parts, as the device has them: all the positions looked up before the walk
    struct Looked {
        uint32_t at[64];
    };
    void top_up(inff::Bits<pos_t>& bb) const { refill(bb); }
    Looked look_ahead(const inff::Bits<pos_t>& bb, const uint32_t* tab, uint32_t held) const {
        Looked c;
        for (uint32_t k = 0; k < 64u; k++)
            c.at[k] = k < held ? inff::literal_at(tab, static_cast<uint32_t>(bb.buf >> k) & 0x7fffu) : 0u;
        return c;
    }
    uint32_t looked(const Looked& c, uint32_t at) const {
        if (at >= 64u) abort();  // a lane that does not exist
        return c.at[at];
    }
    void stored(uint64_t at, uint64_t o, uint32_t len) { memcpy(out + o, in + at, len); }
    void literal(uint64_t o, uint32_t v) { out[o] = static_cast<uint8_t>(v); }
    void match(uint64_t o, uint32_t len, uint32_t dist) {
        for (uint32_t k = 0; k < len; k++) out[o + k] = out[o + k - dist];
    }
    void first_member(uint64_t len, uint32_t crc) {
        first_len = len;
        first_crc = crc;
        gz_seen = true;
    }
    bool member_crc(uint64_t from, uint64_t len, uint32_t crc) const { return crc32(out + from, len) == crc; }
};

template <typename T>
bool get(FILE* f, T* v) { return fread(v, sizeof(T), 1, f) == 1; }

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s vectors.bin\n", argv[0]);
        return 2;
    }
    FILE* f = fopen(argv[1], "rb");
    char magic[8];
    uint32_t count = 0;
    if (!f || fread(magic, 1, 8, f) != 8 || memcmp(magic, "INFVEC1\0", 8) != 0 || !get(f, &count)) {
        fprintf(stderr, "%s: not a vector file\n", argv[1]);
        return 2;
    }
    int bad = 0;
    for (uint32_t v = 0; v < count; v++) {
        uint32_t header_id, gz;
        uint64_t cap, n, m;
        int32_t want;
        if (!get(f, &header_id) || !get(f, &gz) || !get(f, &cap) || !get(f, &want) || !get(f, &n)) return 2;
        uint8_t* comp = exact<uint8_t>(n);
        if (n && fread(comp, 1, n, f) != n) return 2;
        if (!get(f, &m)) return 2;
        std::vector<uint8_t> expect(m);
        if (m && fread(expect.data(), 1, m, f) != m) return 2;
        uint8_t* out = exact<uint8_t>(cap);
        uint64_t got_len = 0;
        int32_t st;
        {
            HostIo io(comp, n, out);
            st = inff::inflate_content(io, header_id, gz != 0, cap, &got_len);
            // the device's second pass: the first member's CRC-32
            if (st == 0 && io.gz_seen && crc32(out, io.first_len) != io.first_crc) st = inff::kBadMsg;
            if (st != 0) got_len = 0;
        }
        bool ok = st == want;
        if (ok && st == 0) ok = got_len == m && (m == 0 || memcmp(out, expect.data(), m) == 0);
        printf("%u status %d len %llu %s\n", v, st, static_cast<unsigned long long>(got_len), ok ? "ok" : "MISMATCH");
        bad += ok ? 0 : 1;
        free(out);
        free(comp);
    }
    fclose(f);
    return bad ? 1 : 0;
}
