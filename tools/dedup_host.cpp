// The content-ID set's decisions on the CPU, under the host sanitizers: runs vectors of calls through
// kopia_amd/csrc/kcdc_dedup_format.h, the header the kernels of kcdc_dedup.hip decide with, in the
// order the device runs them (probe every ID, read every outcome, prefix sums, commit every kept
// key), sequentially and with plain slot words, every table in a heap buffer of exactly the size
// the set has, so a read or write outside one is a sanitizer report.  tests/test_dedup_model.py
// compares the output with the literal loop of tests/dedup_model.py.
//   make build/dedup_host  (g++ -fsanitize=address,undefined -fno-sanitize-recover=all)
//   build/dedup_host < vectors.txt        (or: build/dedup_host vectors.txt)
// Input (text, whitespace separated): "DEDUPVEC1", the vector count, then per vector
//   id_len max_keys ncalls, then per call
//     claim  <prefix> <id_stride> <offset> <n> <hex of offset + n * id_stride bytes, or "-">
//     insert <prefix> <id_stride> <offset> <n> <hex>
//     lookup <prefix> <id_stride> <offset> <n> <hex>
//     clear
//     grow <max_keys>     (a new set of that size takes every key; the vector goes on with it)
//     home <prefix> <hex of id_len bytes>
//   ID i of a call is the id_len bytes at offset + i * id_stride of a buffer of exactly the hex's size.
// Prints per vector "v <index> bytes <kcdc_dedup_bytes> slots <slot count>", then per call
//   claim / insert / grow:  t <status> <new> <stored>, and for claim n lines  k <keep> <first>
//   lookup:                 n lines  l <known>
//   clear:                  c
//   home:                   h <slot>
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "kcdc_dedup_format.h"

using namespace kcdc::dedupfmt;

namespace {
template <typename T>
T* exact(size_t count) { return static_cast<T*>(malloc(count * sizeof(T))); }  // 0: a zero-size block, any access is a report

struct Plain {  // slot words of the sequential program
    static uint64_t load(const uint64_t* p) { return *p; }
    static uint64_t cas(uint64_t* p, uint64_t expect, uint64_t v) {
        const uint64_t old = *p;
        if (old == expect) *p = v;
        return old;
    }
    static void min(uint64_t* p, uint64_t v) {
        if (v < *p) *p = v;
    }
    static void store(uint64_t* p, uint64_t v) { *p = v; }
};

struct Set {
    uint32_t id_len = 0;
    uint64_t max_keys = 0, stored = 0;
    Table t{};
    uint32_t *slot_of = nullptr, *pos = nullptr;
    void open(uint32_t len, uint64_t keys) {
        id_len = len, max_keys = keys, stored = 0;
        t = Table{exact<uint64_t>(slot_count(keys)), slot_count(keys), exact<uint8_t>(keys * key_stride(len)), len};
        slot_of = exact<uint32_t>(keys);
        pos = exact<uint32_t>(keys + 1);
        clear();
    }
    void clear() {
        for (uint64_t s = 0; s < t.nslots; s++) t.slots[s] = kEmpty;
        stored = 0;
    }
    void close() { free(t.slots), free(t.store), free(slot_of), free(pos); }

    // claim / insert / grow: keep and first of exactly n entries, or nullptr
    void claim(const Keys& call, uint32_t n, uint8_t* keep, uint32_t* first) {
        if (refused(stored, n, max_keys)) {
            for (uint32_t i = 0; i < n && keep; i++) keep[i] = 0, first[i] = kKnown;
            printf("t %d 0 %" PRIu64 "\n", kEnospc, stored);
            return;
        }
        for (uint32_t i = 0; i < n; i++) slot_of[i] = static_cast<uint32_t>(probe_claim<Plain>(t, call, i));
        for (uint32_t i = 0; i < n; i++) {
            const uint32_t f = outcome_first<Plain>(t, slot_of[i]);
            pos[i] = f == i;
            if (keep) keep[i] = f == i, first[i] = f;
        }
        uint32_t run = 0;
        for (uint32_t i = 0; i < n; i++) {
            const uint32_t x = pos[i];
            pos[i] = run;
            run += x;
        }
        pos[n] = run;
        for (uint32_t i = 0; i < n; i++) commit_key<Plain>(t, call, i, slot_of[i], static_cast<uint32_t>(stored) + pos[i]);
        stored += run;
        printf("t 0 %u %" PRIu64 "\n", run, stored);
    }
};

int hexval(int c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : -1; }

// a buffer of exactly the hex string's bytes ("-": none)
uint8_t* read_hex(FILE* f, size_t* size) {
    std::string s;
    int c;
    while ((c = fgetc(f)) != EOF && (c == ' ' || c == '\n' || c == '\t' || c == '\r')) {}
    for (; c != EOF && c != ' ' && c != '\n' && c != '\t' && c != '\r'; c = fgetc(f)) s.push_back(static_cast<char>(c));
    if (s == "-") s.clear();
    if (s.size() % 2) return nullptr;
    *size = s.size() / 2;
    uint8_t* b = exact<uint8_t>(*size);
    for (size_t i = 0; i < *size; i++) {
        const int hi = hexval(s[2 * i]), lo = hexval(s[2 * i + 1]);
        if (hi < 0 || lo < 0) return free(b), nullptr;
        b[i] = static_cast<uint8_t>(hi << 4 | lo);
    }
    return b;
}

bool rd(FILE* f, uint64_t* v) { return fscanf(f, "%" SCNu64, v) == 1; }
int bad(const char* what) { return fprintf(stderr, "bad vector file: %s\n", what), 2; }
}  // namespace

int main(int argc, char** argv) {
    FILE* f = argc >= 2 ? fopen(argv[1], "r") : stdin;
    char word[16] = {};
    uint64_t nvec = 0;
    if (!f || fscanf(f, "%15s", word) != 1 || std::string(word) != "DEDUPVEC1" || !rd(f, &nvec)) return bad("header");
    for (uint64_t v = 0; v < nvec; v++) {
        uint64_t id_len = 0, max_keys = 0, ncalls = 0;
        if (!rd(f, &id_len) || !rd(f, &max_keys) || !rd(f, &ncalls)) return bad("truncated");
        if (!valid_shape(static_cast<uint32_t>(id_len), max_keys)) return bad("shape");
        Set set;
        set.open(static_cast<uint32_t>(id_len), max_keys);
        printf("v %" PRIu64 " bytes %" PRIu64 " slots %" PRIu64 "\n", v, layout(set.id_len, max_keys).total, set.t.nslots);
        for (uint64_t c = 0; c < ncalls; c++) {
            if (fscanf(f, "%15s", word) != 1) return bad("truncated");
            const std::string op = word;
            if (op == "clear") {
                set.clear();
                printf("c\n");
            } else if (op == "grow") {
                uint64_t keys = 0;
                if (!rd(f, &keys) || !valid_shape(set.id_len, keys)) return bad("grow");
                Set to;
                to.open(set.id_len, keys);
                to.claim(store_keys(set.t), static_cast<uint32_t>(set.stored), nullptr, nullptr);
                set.close();
                set = to;
            } else if (op == "home") {
                uint64_t prefix = 0;
                size_t size = 0;
                if (!rd(f, &prefix)) return bad("home");
                uint8_t* id = read_hex(f, &size);
                if (!id || size != set.id_len) return bad("home id");
                printf("h %" PRIu64 "\n", home_slot(key_hash(static_cast<uint8_t>(prefix), id), set.t.nslots));
                free(id);
            } else if (op == "claim" || op == "insert" || op == "lookup") {
                uint64_t prefix = 0, stride = 0, offset = 0, n = 0;
                size_t size = 0;
                if (!rd(f, &prefix) || !rd(f, &stride) || !rd(f, &offset) || !rd(f, &n)) return bad("call");
                uint8_t* buf = read_hex(f, &size);
                if (!buf || stride < set.id_len || (n && size < offset + (n - 1) * stride + set.id_len)) return bad("ids");
                const Keys call{buf + offset, stride, set.id_len, static_cast<uint8_t>(prefix), 0};
                const uint32_t n32 = static_cast<uint32_t>(n);
                if (op == "lookup") {
                    for (uint32_t i = 0; i < n32; i++) printf("l %d\n", probe_lookup<Plain>(set.t, call, i) ? 1 : 0);
                } else if (op == "insert") {
                    set.claim(call, n32, nullptr, nullptr);
                } else {
                    uint8_t* keep = exact<uint8_t>(n32);
                    uint32_t* first = exact<uint32_t>(n32);
                    set.claim(call, n32, keep, first);
                    for (uint32_t i = 0; i < n32; i++) printf("k %u %u\n", keep[i], first[i]);
                    free(keep), free(first);
                }
                free(buf);
            } else {
                return bad("unknown call");
            }
        }
        set.close();
    }
    if (f != stdin) fclose(f);
    return 0;
}
