// The pack plan's decisions on the CPU, under the host sanitizers: runs vectors of lengths, masks,
// kept compressed lengths and parameters through kopia_amd/csrc/kcdc_pack_format.h, the header the
// kernels of kcdc_pack.hip decide with, in the order the device runs them (working lengths and the
// total check, keep-or-drop and stored sizes, the prefix sums, the chain of packs, the entries), with
// every table in a heap buffer of exactly the size the call has, so a read or write outside one is
// a sanitizer report.  tests/test_pack_model.py compares the output with the literal loop of
// addToPackUnlocked in tests/pack_model.py.
//   make build/pack_plan_host  (g++ -fsanitize=address,undefined -fno-sanitize-recover=all)
//   build/pack_plan_host vectors.txt
// File (text, whitespace separated): "PACKVEC1", the vector count, then per vector
//   max_pack_size lead open_fill max_total_bytes pack_cap packs_cap header_id
//   ecc data parity max_shard thr_parity_in thr_parity_out thr_blocks_in thr_blocks_out
//   n, then n triples: length keep compressed_length (0: no compressor ran)
// Prints per vector
//   v <index> packs <P> bytes <B> bound_stored <s> bound_packs <p> bound_bytes <b>
//   e <pack> <pack_offset> <packed_length> <original_length> <header_id> <status>    (n lines)
//   p <start> <length> <first> <count>                                              (P lines)
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "kcdc_pack_format.h"

using namespace kcdc;
using namespace kcdc::packfmt;

namespace {
template <typename T>
T* exact(size_t count) { return static_cast<T*>(malloc(count * sizeof(T))); }  // 0: a zero-size block, any access is a report

bool rd(FILE* f, uint64_t* v) { return fscanf(f, "%" SCNu64, v) == 1; }
}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) return fprintf(stderr, "usage: pack_plan_host vectors.txt\n"), 2;
    FILE* f = fopen(argv[1], "r");
    char magic[16] = {};
    uint64_t nvec = 0;
    if (!f || fscanf(f, "%15s", magic) != 1 || std::string(magic) != "PACKVEC1" || !rd(f, &nvec))
        return fprintf(stderr, "bad vector file\n"), 2;
    for (uint64_t v = 0; v < nvec; v++) {
        uint64_t h[15], n64 = 0;
        for (uint64_t& x : h)
            if (!rd(f, &x)) return fprintf(stderr, "truncated vector %" PRIu64 "\n", v), 2;
        if (!rd(f, &n64)) return fprintf(stderr, "truncated vector %" PRIu64 "\n", v), 2;
        Rule r{};
        r.max_pack_size = h[0];
        r.lead = static_cast<uint32_t>(h[1]);
        r.open_fill = static_cast<uint32_t>(h[2]);
        const uint64_t max_total = h[3], pack_cap = h[4], packs_cap = h[5];
        const uint32_t header_id = static_cast<uint32_t>(h[6]), n = static_cast<uint32_t>(n64);
        r.ecc = static_cast<uint32_t>(h[7]);
        r.ep = EccParams{uint32_t(h[8]), uint32_t(h[9]), uint32_t(h[10]), h[11], h[12], h[13], h[14]};

        uint64_t* lens = exact<uint64_t>(n);
        uint8_t* keep = exact<uint8_t>(n);
        uint64_t* clen = exact<uint64_t>(n);
        for (uint32_t i = 0; i < n; i++) {
            uint64_t k = 0;
            if (!rd(f, &lens[i]) || !rd(f, &k) || !rd(f, &clen[i])) return fprintf(stderr, "truncated vector\n"), 2;
            keep[i] = static_cast<uint8_t>(k);
        }
        // plan0: working lengths, the total check
        uint64_t* wlen = exact<uint64_t>(n);
        uint64_t total = 0;
        for (uint32_t i = 0; i < n; i++) total += wlen[i] = chunk_status(lens[i], keep[i] != 0) == kPacked ? lens[i] : 0;
        int32_t refuse = total > max_total ? kEnomem : 0;
        // plan1: keep-or-drop, stored sizes, prefix sums
        uint64_t* E = exact<uint64_t>(size_t(n) + 1);
        uint64_t* C = exact<uint64_t>(size_t(n) + 1);
        uint32_t* hid = exact<uint32_t>(n);
        uint64_t se = 0, sc = 0;
        for (uint32_t i = 0; i < n; i++) {
            const bool room = chunk_status(lens[i], keep[i] != 0) == kPacked && !refuse;
            const bool kept = room && clen[i] != 0 && keep_compressed(clen[i], wlen[i]);
            hid[i] = kept ? header_id : 0;
            E[i] = se;
            C[i] = sc;
            se += room ? stored_size(r, kept ? clen[i] : wlen[i]) : 0;
            sc += room ? 1 : 0;
        }
        E[n] = se;
        C[n] = sc;
        const uint64_t bs = stored_bound(r, max_total, n), bp = packs_bound(r, bs, n);
        // d_packs has packs_cap rows; a vector that gives more than the bound gets no more than that
        const uint64_t nrows = packs_cap < bp + 1 ? packs_cap : bp + 1;
        Row* rows = exact<Row>(nrows);
        const Totals t = place_chain(r, E, C, n, rows, nrows, pack_cap);
        if (t.refuse) refuse = t.refuse;
        printf("v %" PRIu64 " packs %" PRIu64 " bytes %" PRIu64 " bound_stored %" PRIu64 " bound_packs %" PRIu64
               " bound_bytes %" PRIu64 "\n",
               v, t.packs, t.bytes, bs, bp, pack_bytes_bound(r, bs, bp));
        for (uint32_t i = 0; i < n; i++) {
            const Entry e = place_entry(r, E, rows, static_cast<uint32_t>(t.packs), i, lens[i],
                                        chunk_status(lens[i], keep[i] != 0), hid[i], refuse);
            printf("e %u %u %u %u %u %d\n", e.pack, e.pack_offset, e.packed_length, e.original_length, e.header_id,
                   e.status);
        }
        for (uint64_t k = 0; k < t.packs; k++)
            printf("p %" PRIu64 " %" PRIu64 " %u %u\n", rows[k].start, rows[k].length, rows[k].first, rows[k].count);
        free(lens), free(keep), free(clen), free(wlen), free(E), free(C), free(hid), free(rows);
    }
    fclose(f);
    return 0;
}
