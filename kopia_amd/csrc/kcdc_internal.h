// Internal declarations shared by the kcdc host code and the HIP kernels.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>

namespace kcdc {

constexpr int kWindow = 64;  // splitterSlidingWindowSize, repo/splitter/splitter.go:9

struct Tables {
    uint32_t buz[256];      // rollinghash buzhash32 byte table (GenerateHashes(1))
    uint64_t rk_pol = 0;    // rollinghash rabinkarp64 polynomial (RandomPolynomial(1))
    int rk_shift = 0;       // deg(P) - 8
    uint64_t rk_out[256];   // b * x^(8*63) mod P
    uint64_t rk_mod[256];   // (b * x^deg mod P) | (b << deg)
    uint64_t cooked[607];   // Go math/rand rngCooked (rng.go)
};
// rand.New(rand.NewSource(seed)).Read(p[:n]) (Go math/rand, 7 bytes per Int63).
void gorand_read(int64_t seed, uint8_t* p, uint64_t n);
const Tables& tables();

enum Kind : int32_t { kFixed = 0, kBuzhash = 1, kRabinKarp = 2 };

struct Algo {
    const char* name;
    Kind kind;
    bool pooled;
    uint64_t avg;
    uint64_t min_size() const { return kind == kFixed ? avg : avg / 2; }
    uint64_t max_size() const { return kind == kFixed ? avg : avg * 2; }
    uint64_t mask() const { return kind == kFixed ? 0 : avg - 1; }
};
// Registry lookup (repo/splitter/splitter.go:50-86); nullptr if unknown.
const Algo* find_algo(const char* name);
int algo_count();
const Algo* custom_algo(int32_t kind, uint64_t avg);  // interned, nullptr if invalid
int algo_index(const Algo* a);                         // registry index, -1 for custom
const Algo& algo_at(int i);  // sorted by name

// Test knob: lanes per chunk of the content-hash kernels (0 auto, 1, 4).
int& test_hash_lanes();
int test_set_deflate_limit(bool cl, int64_t value);  // kcdc_test_set(KCDC_TEST_DEFLATE_MAXB / _CL_MAXB)
uint64_t& test_id_ring_bytes();  // kcdc_test_set(KCDC_TEST_ID_RING): the writers' ID ring size (0: default)
// kcdc_test_set(KCDC_TEST_CHUNK_GRID): the most workgroups a persistent per-chunk kernel is launched
// with (crypt_units / gcm_units, decode_blocks, inflate, zstd_entropy, zstd_execute, the pack gather,
// the dedup probe / outcome / commit / lookup); 0: no cap.
uint32_t& test_chunk_grid();
inline uint32_t cap_chunk_grid(uint32_t grid) {
    const uint32_t cap = test_chunk_grid();
    return cap != 0 && cap < grid ? cap : grid;
}

// Wrong-output experiment switches compiled into this build (comma-terminated names; "" in
// the product): kcdc_kernels.hip, kcdc_crypt.hip.
const char* ablations_kernels();
const char* ablations_crypt();

// Thread-local error reporting.
int set_error(int code, const std::string& msg);

// ---- kernel launchers (kcdc_kernels.hip) ----
struct DeviceTables;  // per-device copies of the hash tables
const DeviceTables* device_tables(int device, int* err);

struct SplitArgs {
    const uint8_t* const* ptrs;
    const uint64_t* lens;
    uint32_t nstreams;
    uint64_t* cuts;
    uint64_t cuts_cap;
    const uint64_t* cut_base;
    uint64_t* counts;
    const uint64_t* cut_end = nullptr;  // optional per-stream end of the cut range (device)
    const uint64_t* starts = nullptr;   // optional per-stream first chunk start (device; bytes before = history)
    const uint64_t* resume = nullptr;   // optional (with starts): positions below resume[i] are known to hold no
                                        // candidate of stream i's first chunk (a previous round tested them)
};
// Launch the batch splitter for `algo` on `stream` (hipStream_t as void*).
int launch_split_batch(const Algo& algo, const SplitArgs& a, int device, void* stream);
// Single-region first-candidate scan used by the streaming handle:
// bytes [0, len) of `d_buf` are the stream, positions < 0 are zero; returns via
// d_out[0] the first candidate position in [lo, hi] or -1.
// d_scratch (device memory of at least len bytes): a whole workgroup copies the bytes there
// first, then scans them with 8 waves (d_buf is mapped host memory).
int launch_scan_first(const Algo& algo, const uint8_t* d_buf, uint64_t len, int64_t lo, int64_t hi, int64_t* d_out,
                      int device, void* stream, uint8_t* d_scratch);
// The same scan through the device's resident scan server (no launch): 0 and *out = the
// first candidate in [lo, hi] (or -1); 1 = the server is unavailable or busy (launch
// instead); < 0 = error.  d_stage: fine-grained mapped host memory, 256-byte aligned.
int server_scan_first(const Algo& algo, const uint8_t* d_stage, uint64_t len, int64_t lo, int64_t hi, int device,
                      int64_t* out);
void set_scan_server_off(bool off);
uint64_t scan_server_requests();
int launch_fill_prng(uint8_t* d_data, uint64_t stride, uint64_t stream_len, uint32_t nstreams, uint64_t seed,
                     uint64_t first_sid, void* stream);
// Grouped streaming handles: request r scans [lo, hi] of the `len` bytes at base + off.
struct ScanReq {
    uint64_t off;
    int64_t len, lo, hi;
};
int launch_scan_first_batch(const Algo& algo, const uint8_t* d_base, const ScanReq* d_reqs, uint32_t n, int64_t* d_out,
                            int device, void* stream, uint8_t* d_scratch);  // scratch: as base's extent
size_t long_workspace_bytes(const Algo& algo, uint64_t len);
// Several long streams in one launch (segments of all streams scanned together, one
// resolving wave per stream).
size_t long_workspace_bytes_multi(const Algo& algo, const uint64_t* lens, uint32_t m);
int launch_split_long_multi(const Algo& algo, uint32_t m, const uint8_t* const* d_data, const uint64_t* lens,
                            uint64_t* const* d_cuts, const uint64_t* caps, uint64_t* const* d_counts, void* ws,
                            size_t ws_bytes, int device, void* stream);
int launch_split_long(const Algo& algo, const uint8_t* d_data, uint64_t len, uint64_t* d_cuts, uint64_t cuts_cap,
                      uint64_t* d_count, void* ws, size_t ws_bytes, int device, void* stream);

// ---- resumable content hashes (kcdc_hash.hip), for the batching writers
struct HashChain {       // one chunk's keyed BLAKE2 chain, in device memory (128 bytes)
    uint64_t h[8];       // the state (BLAKE2s: the low words)
    uint64_t src;        // the chunk's bytes (device address)
    uint64_t len;        // its length
    uint64_t next;       // message blocks compressed so far; ~0: not started (parameter and key blocks next)
    uint32_t out;        // digest slot
    uint32_t pad[9];
};
static_assert(sizeof(HashChain) == 128, "HashChain is 128 bytes");
// 1 BLAKE2b, 2 BLAKE2s (resumable), 3 another registered name (whole chunks), < 0 unknown; *out_len = digest bytes.
int hash_chain_kind(const char* name, uint32_t* out_len);
// Advance chains d_chains[d_active[0..n)] by at most max_blocks message blocks each; a chain that ends
// writes its digest to d_digests + out * digest_stride.  An entry with kChainNew set starts its chain
// from the record fresh[slot] (src, len, out; may be host-mapped pinned memory, as may d_active and
// d_digests).  Every chunk must start 16-byte aligned and be readable up to its length rounded up
// to 16.
constexpr uint32_t kChainNew = 0x80000000u;
int launch_hash_chains(const char* name, const uint8_t* key, uint32_t key_len, HashChain* d_chains,
                       const HashChain* fresh, const uint32_t* d_active, uint32_t nactive, uint64_t max_blocks,
                       uint8_t* d_digests, uint32_t digest_stride, void* stream);

// ---- content decompression (kcdc_decompress.hip); the compressor registry is kcdc_compress.hip's
// 0 with the name's header ID and whether its stream is S2 framing, or -2 for an unregistered name.
int comp_lookup(const char* name, uint32_t* header_id, bool* s2);
int comp_s2_names(const char** names, int cap);  // the s2-* names (sorted); returns their count
uint64_t decompress_workspace_size(uint64_t total_out_cap_bytes, uint32_t nchunks);
int launch_decompress(uint32_t header_id, const uint8_t* d_comp, const uint64_t* d_offsets, const uint64_t* d_comp_lens,
                      uint32_t nchunks, uint8_t* d_out, const uint64_t* d_out_offsets, const uint64_t* d_out_caps,
                      uint64_t* d_out_lens, int32_t* d_status, void* d_work, uint64_t work_bytes, void* stream);

// ---- inflate (kcdc_inflate.hip): the deflate-*, gzip* and pgzip* names
// 0 with the name's header ID and whether its stream is wrapped in gzip members, -22 for a registered
// name of another format, or -2 for an unregistered name.
int comp_inflate_lookup(const char* name, uint32_t* header_id, bool* gz);
int comp_inflate_names(const char** names, int cap);  // the nine names (sorted); returns their count
uint64_t inflate_workspace_size(uint32_t nchunks);
int launch_inflate(uint32_t header_id, bool gz, const uint8_t* d_comp, const uint64_t* d_offsets,
                   const uint64_t* d_comp_lens, uint32_t nchunks, uint8_t* d_out, const uint64_t* d_out_offsets,
                   const uint64_t* d_out_caps, uint64_t* d_out_lens, int32_t* d_status, void* d_work, uint64_t work_bytes,
                   void* stream);

// ---- zstd decoding (kcdc_zstd.hip): the four zstd* names
// 0 with the name's header ID, -22 for a registered name of another format, or -2 for an
// unregistered name.
int comp_zstd_lookup(const char* name, uint32_t* header_id);
int comp_zstd_names(const char** names, int cap);  // the four names (sorted); returns their count
uint64_t zstd_decode_workspace_size(uint64_t total_out_cap_bytes, uint32_t nchunks);
int launch_zstd_decode(uint32_t header_id, const uint8_t* d_comp, const uint64_t* d_offsets, const uint64_t* d_comp_lens,
                       uint32_t nchunks, uint8_t* d_out, const uint64_t* d_out_offsets, const uint64_t* d_out_caps,
                       uint64_t* d_out_lens, int32_t* d_status, void* d_work, uint64_t work_bytes, void* stream);

// ---- error correction (repo/ecc): parameters and geometry, shared by the host code and kcdc_ecc.hip
#if defined(__HIPCC__)
#define KCDC_HD __host__ __device__
#else
#define KCDC_HD
#endif
constexpr uint32_t kEccLengthSize = 4, kEccCrcSize = 4;              // ecc_rs_crc.go:18-19
constexpr uint32_t kEccSmallData = 6, kEccSmallParity = 2;           // smallFilesDataShards / ParityShards
constexpr uint64_t kEccMinStored = 40;                               // (6 + 2) * (4 + 1): the stored size of 0..2 bytes
constexpr int32_t kEccMaxShardSize = 1 << 24;                        // the largest MaxShardSize this library takes
struct EccParams {  // newReedSolomonCrcECC, ecc_rs_crc.go:37-89
    uint32_t data, parity, max_shard;
    uint64_t thr_parity_in, thr_parity_out, thr_blocks_in, thr_blocks_out;
};
struct EccGeo {  // sizesInfo, ecc_rs_crc.go:401-408
    uint32_t data, parity, shard;
    uint64_t blocks;
    bool pad, small;  // StorePadding; the 6+2 code
    KCDC_HD uint32_t shards() const { return data + parity; }
    KCDC_HD uint64_t rec() const { return uint64_t(shard) + kEccCrcSize; }
    KCDC_HD uint64_t parity_bytes() const { return blocks * parity * rec(); }
};
KCDC_HD inline uint64_t ecc_ceil(uint64_t a, uint64_t b) { return (a + b - 1) / b; }
// computeSizesFromOriginal (ecc_rs_crc.go:91-123); len < 2^32 - 4
KCDC_HD inline EccGeo ecc_geo_original(const EccParams& p, uint64_t len) {
    const uint64_t l = len + kEccLengthSize;
    EccGeo g{};
    if (l <= p.thr_parity_in) {
        g = EccGeo{kEccSmallData, kEccSmallParity, uint32_t(ecc_ceil(l, kEccSmallData)), 1, true, true};
    } else if (l <= p.thr_blocks_in) {
        g = EccGeo{p.data, p.parity, uint32_t(ecc_ceil(l, p.data)), 1, true, false};
    } else {
        g = EccGeo{p.data, p.parity, p.max_shard, ecc_ceil(l, uint64_t(p.data) * p.max_shard), false, false};
    }
    return g;
}
// computeSizesFromStored (ecc_rs_crc.go:125-155)
KCDC_HD inline EccGeo ecc_geo_stored(const EccParams& p, uint64_t stored) {
    EccGeo g{};
    if (stored <= p.thr_parity_out || stored <= p.thr_blocks_out) {
        const bool small = stored <= p.thr_parity_out;
        g.data = small ? kEccSmallData : p.data;
        g.parity = small ? kEccSmallParity : p.parity;
        uint64_t r = ecc_ceil(stored, g.data + g.parity);
        if (r < 1 + kEccCrcSize) r = 1 + kEccCrcSize;
        g.shard = uint32_t(r - kEccCrcSize);
        g.blocks = 1;
        g.pad = true;
        g.small = small;
    } else {
        g = EccGeo{p.data, p.parity, p.max_shard, 0, false, false};
        g.blocks = ecc_ceil(stored, uint64_t(g.shards()) * g.rec());
    }
    return g;
}
// Bytes a len-byte chunk is stored in (computeFinalFileSize, ecc_rs_crc_test.go:171-182).
KCDC_HD inline uint64_t ecc_stored_size(const EccGeo& g, uint64_t len) {
    if (g.pad) return uint64_t(g.shards()) * g.rec() * g.blocks;
    const uint64_t l = len + kEccLengthSize;
    return g.parity_bytes() + l + ecc_ceil(l, g.shard) * kEccCrcSize;
}
// Payload bytes of the data records a stored chunk holds or implies (the logical input, with
// its 4 length bytes), and with that the room its output slot needs: payload - 4.
KCDC_HD inline uint64_t ecc_stored_payload(const EccGeo& g, uint64_t stored) {
    if (g.pad) return uint64_t(g.data) * g.shard;
    if (stored <= g.parity_bytes()) return 0;
    const uint64_t dr = stored - g.parity_bytes(), full = dr / g.rec(), rem = dr % g.rec();
    return full * g.shard + (rem > kEccCrcSize ? rem - kEccCrcSize : 0);
}
bool ecc_known(const char* name);                                        // "REED-SOLOMON-CRC32"
int ecc_params(int32_t overhead_percent, int32_t max_shard_size, EccParams* out);  // 0 or -22 (sets the error)
// Parity rows (parity x data, row-major) of the klauspost/reedsolomon coding matrix.
int ecc_matrix(uint32_t data, uint32_t parity, uint8_t* out);
uint8_t gf_mul(uint8_t a, uint8_t b);
uint8_t gf_inv(uint8_t a);

}  // namespace kcdc
