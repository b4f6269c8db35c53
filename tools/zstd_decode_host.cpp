// The zstd decoder's decisions on the CPU, under the host sanitizers: runs the vector files that
// tests/zstd_vectors.py writes through kopia_amd/csrc/kcdc_zstd_format.h, the header the device
// kernels decide with, as one lane: the index pass, the entropy pass of every compressed block, the
// execute pass and the checksums, with the content, the output slot, the literal room, the sequence
// room, the descriptors and the table context in heap buffers of exactly the size the workspace
// rule grants, so a read or write outside any of them is a sanitizer report.  Every valid and
// corrupt vector runs here before it is sent to a GPU.
//   make build/zstd_decode_host  (g++ -fsanitize=address,undefined -fno-sanitize-recover=all)
//   build/zstd_decode_host vectors.bin
// File (little-endian): "ZSTVEC1\0", u32 count, then per vector: u32 header ID, u64 cap, u64 extra
// descriptors beyond the rule's 4 + cap / 1 KiB, i32 expected status, u64 n, n content bytes, u64 m,
// m expected bytes.  Prints one line per vector; exit status 1 if any status or byte differs.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "kcdc_zstd_format.h"

using namespace kcdc;

namespace {

template <typename T>
T* exact(size_t count) { return static_cast<T*>(malloc(count * sizeof(T))); }  // 0: a zero-size block, any access is a report

// The sequential Io: one lane.
struct HostIo {
    uint32_t lane() const { return 0; }
    uint32_t lanes() const { return 1; }
    bool leader() const { return true; }
    void sync() const {}
    void fence() const {}
    int32_t all(int32_t st) const { return st; }
    void copy(uint8_t* dst, const uint8_t* src, uint32_t len) const {
        for (uint32_t k = 0; k < len; k++) dst[k] = src[k];
    }
    void fill(uint8_t* dst, uint8_t v, uint32_t len) const {
        for (uint32_t k = 0; k < len; k++) dst[k] = v;
    }
    void match(uint8_t* dst, uint32_t len, uint32_t dist) const {
        const uint8_t* src = dst - dist;
        for (uint32_t k = 0; k < len; k++) dst[k] = src[k];
    }
};

// The device's passes over one content; the decoded length into *got.
int32_t decode(const uint8_t* comp, uint64_t n, uint32_t header_id, uint64_t cap64, uint64_t extra, uint8_t* out,
               uint64_t* got) {
    const uint32_t cap = cap64 > 0xffffffffull ? 0xffffffffu : static_cast<uint32_t>(cap64);
    const uint64_t quota = zsf::kQuotaBase + (cap >> zsf::kQuotaShift) + extra;
    zsf::Desc* desc = exact<zsf::Desc>(quota);
    uint8_t* lit_room = exact<uint8_t>(cap);
    zsf::SeqRec* seq_room = exact<zsf::SeqRec>(cap / 3u + 1u);
    zsf::Ctx* ctx = exact<zsf::Ctx>(1);
    zsf::Plan* plan = exact<zsf::Plan>(1);
    HostIo io;
    uint32_t count = 0, total = 0;
    int32_t st = zsf::index_content(comp, n, header_id, cap, desc, quota, &count);
    for (uint32_t b = 0; st == 0 && b < count; b++)
        if (zsf::dget(desc[b], zsf::kFType) == zsf::kTypeComp) st = zsf::entropy_block(io, ctx, comp, desc, b, lit_room, seq_room);
    if (st == 0) st = zsf::execute_content(io, plan, comp, desc, count, lit_room, seq_room, out, cap, &total);
    for (uint32_t b = 0; st == 0 && b < count; b++) {  // the checksum pass
        const zsf::Desc& d = desc[b];
        if (zsf::dget(d, zsf::kFType) != zsf::kTypeFrame || !(zsf::dget(d, zsf::kFInOff) & zsf::kFrameHasSum)) continue;
        const uint64_t h = zsf::xxh64(out + (d.q[2] >> 32), d.q[3]);
        if (static_cast<uint32_t>(h) != static_cast<uint32_t>(d.q[1] >> 32)) st = zsf::kBadMsg;
    }
    *got = st == 0 ? total : 0u;
    free(plan);
    free(ctx);
    free(seq_room);
    free(lit_room);
    free(desc);
    return st;
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
    if (!f || fread(magic, 1, 8, f) != 8 || memcmp(magic, "ZSTVEC1\0", 8) != 0 || !get(f, &count)) {
        fprintf(stderr, "%s: not a vector file\n", argv[1]);
        return 2;
    }
    int bad = 0;
    for (uint32_t v = 0; v < count; v++) {
        uint32_t header_id;
        uint64_t cap, extra, n, m;
        int32_t want;
        if (!get(f, &header_id) || !get(f, &cap) || !get(f, &extra) || !get(f, &want) || !get(f, &n)) return 2;
        uint8_t* comp = exact<uint8_t>(n);
        if (n && fread(comp, 1, n, f) != n) return 2;
        if (!get(f, &m)) return 2;
        std::vector<uint8_t> expect(m);
        if (m && fread(expect.data(), 1, m, f) != m) return 2;
        uint8_t* out = exact<uint8_t>(cap);
        uint64_t got_len = 0;
        const int32_t st = decode(comp, n, header_id, cap, extra, out, &got_len);
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
