// The S2 decoder's decisions on the CPU, under the host sanitizers: decodes the vector files that
// tests/test_s2_vectors.py writes through kopia_amd/csrc/kcdc_s2_format.h, the header the device
// kernels decide with, in exactly-sized heap buffers, so a read or write outside a content, its
// descriptors or its slot is a sanitizer report.  Every valid and corrupt vector runs here before
// it is sent to a GPU.
//   make build/s2_decode_host      (g++ -fsanitize=address,undefined -fno-sanitize-recover=all)
//   build/s2_decode_host vectors.bin
// File (little-endian): "S2VEC1\0\0", u32 count, then per vector: u32 header ID, u64 cap,
// u64 descriptor room, i32 expected status, u64 n, n content bytes, u64 m, m expected bytes.
// Prints one line per vector; exit status 1 if any status or byte differs from the expectation.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "kcdc_s2_format.h"
#include "kcdc_wave.h"

using namespace kcdc;

namespace {

uint32_t crc32c(const uint8_t* p, uint64_t n) {
    uint32_t c = 0xFFFFFFFFu;
    for (uint64_t i = 0; i < n; i++) {
        c ^= p[i];
        for (int k = 0; k < 8; k++) c = (c >> 1) ^ (compdev::kCrc32cPoly & (0u - (c & 1u)));
    }
    return c ^ 0xFFFFFFFFu;
}

// The device's passes for one content: index, then every block, then every CRC.
int32_t decode_content(const uint8_t* comp, uint64_t n, uint32_t header_id, uint8_t* out, uint64_t cap,
                       s2f::Desc* descs, uint64_t max_desc, uint64_t* out_len) {
    uint32_t count = 0;
    uint64_t total = 0;
    *out_len = 0;
    int32_t st = s2f::index_content(comp, n, header_id, cap, 0, 0, 0, descs, max_desc, &count, &total);
    if (st != 0) return st;
    for (uint32_t k = 0; k < count; k++) {
        const s2f::Desc& d = descs[k];
        if (d.in_off + d.in_len > n || d.out_off + d.out_len > cap) abort();  // the index pass's promise
        if (d.content & s2f::kDescRaw) {
            if (d.in_len != d.out_len) abort();
            memcpy(out + d.out_off, comp + d.in_off, d.out_len);
        } else {
            // the block in a buffer of its own size: the walk may not read past it
            uint8_t* blk = static_cast<uint8_t*>(malloc(d.in_len ? d.in_len : 1));
            uint8_t* dst = static_cast<uint8_t*>(malloc(d.out_len ? d.out_len : 1));
            memcpy(blk, comp + d.in_off, d.in_len);
            const int32_t r = s2f::decode_block_serial(blk, d.in_len, dst, d.out_len);
            if (r == 0) memcpy(out + d.out_off, dst, d.out_len);
            free(blk);
            free(dst);
            if (r != 0) return r;
        }
        if (s2f::mask_crc(crc32c(out + d.out_off, d.out_len)) != d.crc) return s2f::kBadMsg;
    }
    *out_len = total;
    return 0;
}

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
    if (!f || fread(magic, 1, 8, f) != 8 || memcmp(magic, "S2VEC1\0\0", 8) != 0 || !get(f, &count)) {
        fprintf(stderr, "%s: not a vector file\n", argv[1]);
        return 2;
    }
    int bad = 0;
    for (uint32_t v = 0; v < count; v++) {
        uint32_t header_id;
        uint64_t cap, room, n, m;
        int32_t want;
        if (!get(f, &header_id) || !get(f, &cap) || !get(f, &room) || !get(f, &want) || !get(f, &n)) return 2;
        uint8_t* comp = static_cast<uint8_t*>(malloc(n ? n : 1));
        if (n && fread(comp, 1, n, f) != n) return 2;
        if (!get(f, &m)) return 2;
        std::vector<uint8_t> expect(m);
        if (m && fread(expect.data(), 1, m, f) != m) return 2;
        uint8_t* out = static_cast<uint8_t*>(malloc(cap ? cap : 1));
        s2f::Desc* descs = static_cast<s2f::Desc*>(malloc(room ? room * sizeof(s2f::Desc) : 1));
        uint64_t got_len = 0;
        const int32_t st = decode_content(comp, n, header_id, out, cap, descs, room, &got_len);
        bool ok = st == want;
        if (ok && st == 0) ok = got_len == m && (m == 0 || memcmp(out, expect.data(), m) == 0);
        printf("%u status %d len %llu %s\n", v, st, static_cast<unsigned long long>(got_len), ok ? "ok" : "MISMATCH");
        bad += ok ? 0 : 1;
        free(descs);
        free(out);
        free(comp);
    }
    fclose(f);
    return bad ? 1 : 0;
}
