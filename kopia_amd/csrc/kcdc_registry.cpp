// Splitter registry — repo/splitter/splitter.go:8-89.
//
// The reference keeps an unexported name -> Factory map (`splitterFactories`,
// :50-81) and exposes SupportedAlgorithms (:32-42, sorted), GetFactory (:84-86)
// and DefaultAlgorithm (:89).  Names are persisted in repository configs and
// policies, so this table must list exactly the reference's 23 names with the
// same parameters; new names must never be introduced.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <deque>
#include <vector>
#include <mutex>
#include <string>

#include "kcdc_internal.h"

namespace kcdc {
namespace {

constexpr uint64_t KiB = 1024, MiB = 1024 * 1024;

// Sorted by std::strcmp order == Go sort.Strings order (byte-wise).
const Algo kAlgos[] = {
    {"DYNAMIC", kBuzhash, false, 4 * MiB},  // splitter.go:80 (legacy name, not pooled)
    {"DYNAMIC-128K-BUZHASH", kBuzhash, true, 128 * KiB},
    {"DYNAMIC-128K-RABINKARP", kRabinKarp, true, 128 * KiB},
    {"DYNAMIC-1M-BUZHASH", kBuzhash, true, 1 * MiB},
    {"DYNAMIC-1M-RABINKARP", kRabinKarp, true, 1 * MiB},
    {"DYNAMIC-256K-BUZHASH", kBuzhash, true, 256 * KiB},
    {"DYNAMIC-256K-RABINKARP", kRabinKarp, true, 256 * KiB},
    {"DYNAMIC-2M-BUZHASH", kBuzhash, true, 2 * MiB},
    {"DYNAMIC-2M-RABINKARP", kRabinKarp, true, 2 * MiB},
    {"DYNAMIC-4M-BUZHASH", kBuzhash, true, 4 * MiB},
    {"DYNAMIC-4M-RABINKARP", kRabinKarp, true, 4 * MiB},
    {"DYNAMIC-512K-BUZHASH", kBuzhash, true, 512 * KiB},
    {"DYNAMIC-512K-RABINKARP", kRabinKarp, true, 512 * KiB},
    {"DYNAMIC-8M-BUZHASH", kBuzhash, true, 8 * MiB},
    {"DYNAMIC-8M-RABINKARP", kRabinKarp, true, 8 * MiB},
    {"FIXED", kFixed, false, 4 * MiB},  // splitter.go:76 (legacy name, not pooled)
    {"FIXED-128K", kFixed, true, 128 * KiB},
    {"FIXED-1M", kFixed, true, 1 * MiB},
    {"FIXED-256K", kFixed, true, 256 * KiB},
    {"FIXED-2M", kFixed, true, 2 * MiB},
    {"FIXED-4M", kFixed, true, 4 * MiB},
    {"FIXED-512K", kFixed, true, 512 * KiB},
    {"FIXED-8M", kFixed, true, 8 * MiB},
};
constexpr int kNumAlgos = sizeof(kAlgos) / sizeof(kAlgos[0]);

thread_local std::string t_error;

// Interned custom parameterisations (kcdc_custom_algorithm); never freed so the
// returned names and Algo pointers stay valid for the life of the process.
std::mutex g_custom_mu;
std::deque<std::string> g_custom_names;
std::deque<Algo> g_custom;

}  // namespace

const Algo* find_algo(const char* name) {
    if (!name) return nullptr;
    for (const Algo& a : kAlgos)
        if (std::strcmp(a.name, name) == 0) return &a;
    std::lock_guard<std::mutex> lk(g_custom_mu);
    for (const Algo& a : g_custom)
        if (std::strcmp(a.name, name) == 0) return &a;
    return nullptr;
}

const Algo* custom_algo(int32_t kind, uint64_t avg) {
    if (kind != kFixed && kind != kBuzhash && kind != kRabinKarp) return nullptr;
    if (kind == kFixed ? avg < 1 : (avg < 2 || (avg & (avg - 1)) != 0 || avg > (uint64_t(1) << 31))) return nullptr;
    static const char* kKindName[] = {"fixed", "buzhash", "rabinkarp"};
    const std::string nm = std::string("kcdc:") + kKindName[kind] + ":" + std::to_string(avg);
    std::lock_guard<std::mutex> lk(g_custom_mu);
    for (const Algo& a : g_custom)
        if (nm == a.name) return &a;
    g_custom_names.push_back(nm);
    g_custom.push_back(Algo{g_custom_names.back().c_str(), static_cast<Kind>(kind), false, avg});
    return &g_custom.back();
}

int algo_index(const Algo* a) {
    const ptrdiff_t i = a - kAlgos;
    return (i >= 0 && i < kNumAlgos) ? static_cast<int>(i) : -1;
}
int algo_count() { return kNumAlgos; }
const Algo& algo_at(int i) { return kAlgos[i]; }

int set_error(int code, const std::string& msg) {
    t_error = msg;
    return code;
}
const char* last_error_cstr() { return t_error.c_str(); }

// ---------------------------------------------------------------- repo/ecc: registry and parameters
// One registered algorithm (RegisterAlgorithm, ecc_rs_crc.go:414-418).
bool ecc_known(const char* name) { return name && std::strcmp(name, "REED-SOLOMON-CRC32") == 0; }

namespace {
// computeShards (ecc_utils.go:5-20).  float where the reference has float32, double where it
// widens (applyPercent): other widths give other shard counts at some overheads.
int ecc_between(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
int ecc_apply_percent(int val, float percent) {
    return static_cast<int>(std::floor(static_cast<double>(val) * static_cast<double>(percent)));
}
void ecc_compute_shards(float space_overhead, int* data, int* parity) {
    *data = 128;
    *parity = ecc_between(ecc_apply_percent(*data, space_overhead / 100.0f), 1, 128);
    if (*parity == 1) {
        *parity = 2;
        *data = ecc_between(ecc_apply_percent(*parity, 100.0f / space_overhead), 128, 254);
    }
}

// GF(2^8), polynomial 0x11d, generator 2 (klauspost/reedsolomon galois.go).
struct GfTables {
    uint8_t exp[512];
    uint8_t log[256];
    GfTables() {
        int x = 1;
        for (int i = 0; i < 255; i++) {
            exp[i] = static_cast<uint8_t>(x);
            log[x] = static_cast<uint8_t>(i);
            x <<= 1;
            if (x & 0x100) x ^= 0x11d;
        }
        for (int i = 255; i < 512; i++) exp[i] = exp[i - 255];
        log[0] = 0;
    }
};
const GfTables& gf() {
    static const GfTables t;
    return t;
}
uint8_t gf_exp(uint8_t a, int n) {  // galExp: a^n, 0^0 = 1
    if (n == 0) return 1;
    if (a == 0) return 0;
    return gf().exp[(static_cast<int>(gf().log[a]) * n) % 255];
}
}  // namespace

uint8_t gf_mul(uint8_t a, uint8_t b) { return (a && b) ? gf().exp[gf().log[a] + gf().log[b]] : 0; }
uint8_t gf_inv(uint8_t a) { return gf().exp[255 - gf().log[a]]; }

int ecc_params(int32_t overhead_percent, int32_t max_shard_size, EccParams* out) {
    if (!out) return set_error(-22, "null argument");
    if (overhead_percent < 1 || overhead_percent > 100) return set_error(-22, "ECC overhead must be 1..100 percent");
    if (max_shard_size < 0 || max_shard_size > kEccMaxShardSize)
        return set_error(-22, "ECC max shard size must be 0 (by overhead) or 1..2^24");
    int ms = max_shard_size;
    if (ms == 0) ms = overhead_percent == 1 ? 1024 : overhead_percent == 2 ? 512 : overhead_percent == 3 ? 256
                      : overhead_percent <= 6 ? 128 : 64;
    float free_overhead = static_cast<float>(overhead_percent) - 400.0f / static_cast<float>(ms);
    if (!(free_overhead >= 0.01f)) free_overhead = 0.01f;
    int d = 0, p = 0;
    ecc_compute_shards(free_overhead, &d, &p);
    out->data = static_cast<uint32_t>(d);
    out->parity = static_cast<uint32_t>(p);
    out->max_shard = static_cast<uint32_t>(ms);
    out->thr_parity_in = 2ull * kEccCrcSize * (d + p);
    out->thr_parity_out = uint64_t(kEccSmallData + kEccSmallParity) *
                          (kEccCrcSize + ecc_ceil(out->thr_parity_in, kEccSmallData));
    out->thr_blocks_in = uint64_t(d) * ms;
    out->thr_blocks_out = uint64_t(d + p) * (kEccCrcSize + uint64_t(ms));
    return 0;
}

// buildMatrix (klauspost/reedsolomon reedsolomon.go): V[r][c] = r^c, M = V * (V[0:data])^-1; the
// top data rows of M are the identity, the rest are the parity rows returned here.
int ecc_matrix(uint32_t data, uint32_t parity, uint8_t* out) {
    if (!out || data < 1 || parity < 1 || data + parity > 256) return set_error(-22, "coding matrix: 1 <= data, parity and data + parity <= 256");
    const uint32_t n = data + parity;
    std::vector<uint8_t> v(size_t(n) * data), inv(size_t(data) * data, 0), top(size_t(data) * data);
    for (uint32_t r = 0; r < n; r++)
        for (uint32_t c = 0; c < data; c++) v[size_t(r) * data + c] = gf_exp(static_cast<uint8_t>(r), static_cast<int>(c));
    std::copy(v.begin(), v.begin() + size_t(data) * data, top.begin());
    for (uint32_t i = 0; i < data; i++) inv[size_t(i) * data + i] = 1;
    for (uint32_t c = 0; c < data; c++) {  // Gauss-Jordan on [top | inv]
        uint32_t piv = c;
        while (piv < data && top[size_t(piv) * data + c] == 0) piv++;
        if (piv == data) return set_error(-22, "coding matrix: singular Vandermonde block");
        if (piv != c)
            for (uint32_t k = 0; k < data; k++) {
                std::swap(top[size_t(piv) * data + k], top[size_t(c) * data + k]);
                std::swap(inv[size_t(piv) * data + k], inv[size_t(c) * data + k]);
            }
        const uint8_t s = gf_inv(top[size_t(c) * data + c]);
        for (uint32_t k = 0; k < data; k++) {
            top[size_t(c) * data + k] = gf_mul(top[size_t(c) * data + k], s);
            inv[size_t(c) * data + k] = gf_mul(inv[size_t(c) * data + k], s);
        }
        for (uint32_t r = 0; r < data; r++) {
            const uint8_t f = top[size_t(r) * data + c];
            if (r == c || f == 0) continue;
            for (uint32_t k = 0; k < data; k++) {
                top[size_t(r) * data + k] ^= gf_mul(f, top[size_t(c) * data + k]);
                inv[size_t(r) * data + k] ^= gf_mul(f, inv[size_t(c) * data + k]);
            }
        }
    }
    for (uint32_t r = 0; r < parity; r++)
        for (uint32_t c = 0; c < data; c++) {
            uint8_t acc = 0;
            for (uint32_t k = 0; k < data; k++) acc ^= gf_mul(v[size_t(data + r) * data + k], inv[size_t(k) * data + c]);
            out[size_t(r) * data + c] = acc;
        }
    return 0;
}

}  // namespace kcdc
