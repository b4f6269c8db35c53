/*
 * kcdc.h — C ABI of the MI355X-native content-defined-chunking splitter for
 * Kopia (library: kopia_amd/libkcdc.so, built for gfx950).
 *
 * This is the drop-in boundary for Kopia's `repo/splitter` package.  Every
 * entry point below names the reference interface it replaces
 * (paths relative to the kopia/kopia tree).  Plain pointers and sizes only;
 * no torch or HIP types appear in the signatures (streams are passed as
 * `void*` holding a hipStream_t, or NULL for the library's own stream).
 *
 * Semantics are bit-exact with the reference Go splitters: for any input bytes
 * and any slicing of them, the split points are the ones Kopia computes.
 *
 * Errors: functions returning `int` return KCDC_OK (0) or a negative KCDC_E*
 * code and set a thread-local message readable with kcdc_last_error().  There
 * is NO silent CPU fallback: if the GPU path cannot run, the call fails.
 */
#ifndef KCDC_H
#define KCDC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KCDC_OK 0
#define KCDC_ENOENT (-2)     /* unknown splitter name */
#define KCDC_EIO (-5)        /* HIP runtime / kernel error */
#define KCDC_ENOMEM (-12)
#define KCDC_EINVAL (-22)
#define KCDC_ENODEV (-19)    /* no usable gfx950 device */
#define KCDC_EOVERFLOW (-75) /* caller-provided cut capacity too small */
#define KCDC_EFBIG (-27)     /* chunk too long to encrypt (>= 1 GiB) */
#define KCDC_EBADMSG (-74)   /* sealed chunk failed authentication */
#define KCDC_ENOSPC (-28)    /* the content-ID set cannot take the call's IDs */

/* counts[i] value of every stream of a batch launch that could not complete on the
 * device (a wave gave up waiting in the work queue): the launch's cut lists are invalid.
 * The _host entry points return KCDC_EIO instead. */
#define KCDC_COUNT_FAILED UINT64_MAX

#define KCDC_KIND_FIXED 0
#define KCDC_KIND_BUZHASH 1
#define KCDC_KIND_RABINKARP 2

/* Parameters behind a registered name.
 * Reference: newBuzHash32SplitterFactory repo/splitter/splitter_buzhash32.go:73-86,
 * newRabinKarp64SplitterFactory splitter_rabinkarp64.go:73-83, Fixed splitter_fixed.go:33-37. */
typedef struct kcdc_algo_info {
    int32_t kind;      /* KCDC_KIND_* */
    int32_t pooled;    /* 1 if the reference wraps the factory in pooled() (splitter.go:51-73) */
    uint64_t avg;      /* average chunk size (FIXED: chunk length) */
    uint64_t min_size; /* avg/2 (FIXED: chunk length) */
    uint64_t max_size; /* 2*avg (FIXED: chunk length) == MaxSegmentSize() */
    uint64_t mask;     /* avg-1 (FIXED: 0) */
} kcdc_algo_info;

/* ------------------------------------------------------------ diagnostics */
const char* kcdc_last_error(void);
const char* kcdc_version(void);
/* Number of visible gfx950 devices (0 on a machine without one). */
int kcdc_device_count(void);

/* --------------------------------------------------------------- registry */
/* SupportedAlgorithms() — repo/splitter/splitter.go:32-42 (sorted names).
 * Writes up to `cap` name pointers (static storage) and returns the total count. */
int kcdc_supported_algorithms(const char** names, int cap);
/* DefaultAlgorithm — repo/splitter/splitter.go:89 ("DYNAMIC-4M-BUZHASH"). */
const char* kcdc_default_algorithm(void);
/* GetFactory(name) != nil — repo/splitter/splitter.go:84-86.  Returns KCDC_OK or KCDC_ENOENT. */
int kcdc_lookup(const char* name, kcdc_algo_info* info);
/* Factory().MaxSegmentSize() — splitter_buzhash32.go:69-71 / splitter_rabinkarp64.go:69-71 /
 * splitter_fixed.go:29-31.  Returns < 0 (KCDC_ENOENT) for unknown names. */
int64_t kcdc_max_segment_size(const char* name);
/* Name for a NON-registered parameterisation, mirroring the unexported factory
 * constructors the reference tests call directly: newBuzHash32SplitterFactory(avg)
 * (splitter_buzhash32.go:73), newRabinKarp64SplitterFactory(avg)
 * (splitter_rabinkarp64.go:73), Fixed(length) (splitter_fixed.go:33); see
 * repo/splitter/splitter_test.go:27-52.  `avg` must be a power of two >= 2 for
 * the rolling kinds (mask = avg-1), >= 1 for FIXED.  Returns an interned name
 * (static storage, never in kcdc_supported_algorithms) accepted by every
 * name-taking entry point, or NULL (KCDC_EINVAL). */
const char* kcdc_custom_algorithm(int32_t kind, uint64_t avg);
/* Upper bound on the number of chunks of a `stream_len`-byte stream (every chunk
 * but the last is >= min size): size cut arrays with it. */
uint64_t kcdc_cut_capacity(const char* name, uint64_t stream_len);

/* Rolling-hash constants as derived by the library (buzhash32 byte table,
 * Rabin-Karp polynomial and out/mod tables; rollinghash v4.0.0, go.mod:13).
 * Any pointer may be NULL.  Host-only: works without a GPU. */
int kcdc_tables(uint32_t* buzhash256, uint64_t* rabin_pol, uint64_t* rabin_out256, uint64_t* rabin_mod256);

/* ------------------------------------------------ streaming Splitter handle
 * Mirrors `type Splitter interface` (repo/splitter/splitter.go:20-29) and
 * `type Factory func() Splitter` (:45).  One handle per object writer; calls on
 * one handle must be serialised by the caller (objectWriter.mu,
 * repo/object/object_writer.go:114), handles are independent of each other.
 * `b` is borrowed for the call only (object_writer.go:121-129). */
typedef struct kcdc_splitter kcdc_splitter;
/* GetFactory(name)() — NULL on unknown name or no device (see kcdc_last_error). */
kcdc_splitter* kcdc_splitter_new(const char* name, int device);
/* NextSplitPoint(b) — returns n in 1..len (split AFTER byte n, n bytes consumed),
 * -1 if no split point (all consumed), or a KCDC_E* code (< -1) on failure. */
int64_t kcdc_splitter_next(kcdc_splitter* s, const uint8_t* b, size_t len);
/* MaxSegmentSize() */
int64_t kcdc_splitter_max_segment_size(const kcdc_splitter* s);
/* Reset() — splitter_buzhash32.go:20-24: back to the 64-zero window, count 0. */
void kcdc_splitter_reset(kcdc_splitter* s);
/* Close() — splitter_pool.go:18-22: Reset and return to the name's pool (pooled
 * names) or free.  The handle must not be used afterwards. */
void kcdc_splitter_close(kcdc_splitter* s);

/* ------------------------------------------------ grouped streaming handles
 * Kopia runs many object writers at once (snapshot/upload/upload.go:769-782),
 * each with its own Splitter fed 64 KiB slices (upload.go:394-407).  A group
 * batches the GPU work of all its handles' concurrent NextSplitPoint calls into
 * one launch: each call stages its slice into pinned memory from its own thread
 * and blocks until the group's launch returns its answer (same semantics and
 * results as kcdc_splitter_next on a private handle).  The group thread waits up
 * to `max_wait_us` for more calls (0: ship whatever is there) and takes at most
 * `max_batch` calls per launch (0: 256).  One name per group (a repository uses
 * one splitter).  Handles come from kcdc_group_splitter and are released with
 * kcdc_splitter_close.  kcdc_group_free may come first: the group then lives on
 * until its last handle is closed (no handle may be created after it). */
typedef struct kcdc_group kcdc_group;
kcdc_group* kcdc_group_new(const char* name, int device, uint32_t max_batch, uint32_t max_wait_us);
kcdc_splitter* kcdc_group_splitter(kcdc_group* g);
void kcdc_group_free(kcdc_group* g);

/* ------------------------------------------------ batching object writers
 * The writer-level form of the streaming handle: objectWriter.Write
 * (repo/object/object_writer.go:113-139) hands each 64 KiB slice (snapshot/upload/
 * upload.go:394-407) to kcdc_bw_write, which only copies it into pinned staging.  A batcher
 * thread ships every writer's staged bytes in one round (H2D, one batch-splitter launch over
 * all writers, cut lists back) once `round_bytes` are staged (0: 256 MiB) or `max_wait_us`
 * after the first staged byte (0: 2000).  Cut decisions therefore arrive later than the
 * bytes: kcdc_bw_cuts returns the FINAL cut offsets found so far (absolute offsets in the
 * object, strictly increasing, each a chunk end), and after kcdc_bw_finish (the object's
 * Close/Result: blocks until every byte is split) the remaining ones including the trailing
 * chunk's end.  The sequence is exactly the cuts of one NextSplitPoint pass over the whole
 * object, however it was sliced.  The writer must keep the bytes of its unflushed chunks
 * (objectWriter already buffers them in gather.WriteBuffer) and flush each chunk when its cut
 * arrives.  Calls on one writer are serialised by the caller; writers are independent.
 * kcdc_bw_write blocks while half a round of the writer's bytes is still unshipped.
 *
 * Devices: kcdc_bw_batcher_new_devices spreads the writers over a device set (`devices`, or
 * every device when NULL / ndev <= 0; an index may repeat, e.g. two logical devices on one
 * GPU).  Each device has its own round thread, streams and arenas; kcdc_bw_open assigns a writer
 * to the device with the least load (the bytes of its open writers, each counted as the larger
 * of its size hint and its bytes written: kcdc_bw_open_hint passes the object's expected size,
 * e.g. the file size the uploader knows, snapshot/upload/upload.go:769-782).  kcdc_bw_device
 * returns the writer's position in the device list.
 * Device memory: every open writer holds two arenas of about max_size + 4 x (round_bytes / 8 +
 * 4 MiB) bytes each (152 MiB at the defaults); kcdc_bw_open fails with KCDC_ENOMEM when the
 * device cannot hold them.
 * A freed writer's arenas are kept for the next kcdc_bw_open (hipMalloc/hipFree per object would
 * serialise on the device): at most as many pairs as writers were open at once, all given back
 * when a kcdc_bw_open would otherwise fail with KCDC_ENOMEM, and at kcdc_bw_batcher_free.
 * kcdc_bw_batcher_free ships what is staged, then fails every writer call still blocked in it
 * (KCDC_EINVAL) and waits for those calls to return; writers not freed before it stay valid for
 * kcdc_bw_free only.  A writer call that starts while or after kcdc_bw_batcher_free runs returns
 * KCDC_EINVAL without touching the freed batcher (its lifetime state is refcounted by its
 * writers), and kcdc_bw_free of such a writer waits until the batcher has let it go. */
typedef struct kcdc_bw_batcher kcdc_bw_batcher;
typedef struct kcdc_bw kcdc_bw;
kcdc_bw_batcher* kcdc_bw_batcher_new(const char* name, int device, uint64_t round_bytes, uint32_t max_wait_us);
kcdc_bw_batcher* kcdc_bw_batcher_new_devices(const char* name, const int* devices, int ndev, uint64_t round_bytes,
                                             uint32_t max_wait_us);
int kcdc_bw_batcher_devices(const kcdc_bw_batcher* b);  /* devices in the set */
void kcdc_bw_batcher_free(kcdc_bw_batcher* b);
kcdc_bw* kcdc_bw_open(kcdc_bw_batcher* b);        /* Factory() for one object */
kcdc_bw* kcdc_bw_open_hint(kcdc_bw_batcher* b, uint64_t size_hint);
int kcdc_bw_device(const kcdc_bw* w);             /* the writer's device (position in the list) */
int kcdc_bw_write(kcdc_bw* w, const uint8_t* p, size_t len);
int64_t kcdc_bw_cuts(kcdc_bw* w, uint64_t* out, uint64_t cap); /* final cuts taken (<= cap), or KCDC_E* */
int kcdc_bw_finish(kcdc_bw* w);
void kcdc_bw_free(kcdc_bw* w);
/* Content IDs (round 5): name every final chunk on the device, from the bytes the rounds already
 * hold, as the content manager does after the object writer flushes it
 * (repo/object/object_writer.go:186-227 -> repo/content/content_manager.go:812, hashData):
 * kcdc_bw_batcher_hash selects a registered hash name (kcdc_hash_algorithms; the repository's
 * hasher, hashing.go:51 defaults to BLAKE2B-256-128) and its HMAC secret, before the first writer
 * opens.  Then kcdc_bw_cuts_ids replaces kcdc_bw_cuts: it returns up to cap final cuts in order, each
 * with its chunk's digest (kcdc_hash_size bytes at ids + i * id_stride), as soon as the digests of
 * every chunk up to it are known; kcdc_bw_finish also waits for the last chunk's digest.  BLAKE2
 * names hash in slices of 256 KiB per chunk per step (a chunk is one chain of compressions), the
 * others whole chunks per step, on a hash thread of their own.  Device memory: an ID ring of
 * max(64 x round_bytes, 1 GiB) per device holds the chunks until they are named (a chunk is one
 * dependent chain, so the naming rate grows with the chunks in flight).  FIXED names: KCDC_EINVAL
 * (their writers stage no bytes on the device). */
int kcdc_bw_batcher_hash(kcdc_bw_batcher* b, const char* hash_name, const uint8_t* key, uint32_t key_len);
int64_t kcdc_bw_cuts_ids(kcdc_bw* w, uint64_t* cuts, uint8_t* ids, uint32_t id_stride, uint64_t cap);
int64_t kcdc_bw_rounds(const kcdc_bw_batcher* b); /* rounds shipped so far (test hook) */
/* Observability (summed over the batcher's devices; the span and busy seconds are the largest
 * device's): out[0..n) = rounds, bytes shipped, seconds the round thread spent building and
 * issuing rounds, seconds it waited for the device, then the device seconds of the rounds' gathers
 * (new bytes over PCIe into the writers' arenas) and of their splits (metadata in, splitter
 * launch, cut lists out), from HIP events, then the device span of all rounds and the seconds of
 * it in which a gather or a split ran, then the round thread's seconds per phase (collecting the
 * writers' blocks, placing them in the arenas, issuing the gather, waiting for the previous round,
 * issuing the split), then the round thread's seconds waiting for a round's worth of staged bytes,
 * and the writers' seconds (summed over writers) blocked on their staging cap and getting a pinned
 * staging block, then the pinned blocks allocated because the pool was empty and the round
 * thread's seconds acquiring the batcher's mutex to apply a finished round, then (content IDs)
 * the chunks named, the hash steps issued and their device seconds, the round thread's seconds
 * waiting for ID ring space, the hash thread's seconds with no step to issue, and the chains
 * advanced summed over steps.  Returns 24. */
int kcdc_bw_stats(kcdc_bw_batcher* b, double* out, int n);

/* ------------------------------------------------------ batch (hot path)
 * Split `nstreams` independent streams in one launch; every stream starts from
 * a fresh splitter (the pool's Reset-on-Close, splitter_pool.go:18-22).
 * Output for stream i: counts[i] chunk END offsets written to
 * cuts[cut_base[i] .. cut_base[i]+counts[i]), strictly increasing, the last one
 * equal to lens[i] (the trailing chunk `Result()` flushes,
 * repo/object/object_writer.go:264-277).  An empty stream yields 0 entries.
 * Capacity for stream i is cut_base[i+1]-cut_base[i] (last: `cuts_cap`-cut_base[i]);
 * size it with kcdc_cut_capacity().  counts[i] always receives the TRUE number of
 * chunks; entries beyond the capacity are not written, so counts[i] > capacity
 * signals overflow (the _host variant returns KCDC_EOVERFLOW).
 *
 * _device: every pointer (the array of stream pointers, lens, cuts, cut_base,
 * counts) is device memory on the current device; the call is asynchronous on
 * `hip_stream` (NULL = legacy default stream) except for error checking of
 * the launch.  A launch that fails on the device sets every counts[i] to
 * KCDC_COUNT_FAILED (no partial results are ever reported as complete).  Stream bytes may have any alignment.  Each launch takes one of 64
 * per-device queue workspaces in turn; a launch that reuses a workspace still in
 * use by another stream waits for it (an event), so any number may be in flight. */
int kcdc_split_batch_device(const char* name, const uint8_t* const* d_ptrs, const uint64_t* d_lens,
                            uint32_t nstreams, uint64_t* d_cuts, uint64_t cuts_cap, const uint64_t* d_cut_base,
                            uint64_t* d_counts, void* hip_stream);

/* _host: host buffers in, host cut lists out.  Streams are copied H2D in groups
 * of <= 1 GiB (the HIP runtime stages pageable memory; buffers the caller
 * allocated pinned are DMA'd directly), each group split like
 * kcdc_split_files_device (large streams through the long-stream path), and the
 * cut lists copied back.  Synchronous, PCIe-bound.  This is the
 * path the Go cgo shim calls. */
int kcdc_split_batch_host(const char* name, const uint8_t* const* h_ptrs, const uint64_t* lens, uint32_t nstreams,
                          uint64_t* cuts, uint64_t cuts_cap, const uint64_t* cut_base, uint64_t* counts, int device);
/* The same over a device set (`devices`, repeats allowed; NULL / ndev <= 0: every device): the
 * streams are spread by bytes with kcdc_lpt_assign and each device splits its share from a host
 * thread of its own (no collectives: SURVEY.md §8e).  Same output contract as one device. */
int kcdc_split_batch_host_devices(const char* name, const int* devices, int ndev, const uint8_t* const* h_ptrs,
                                  const uint64_t* lens, uint32_t nstreams, uint64_t* cuts, uint64_t cuts_cap,
                                  const uint64_t* cut_base, uint64_t* counts);
/* Longest-processing-time-first assignment by bytes (largest stream first, each to the least
 * loaded of `ndev` devices, ties to the lower index): dev_of[i] = position of stream i's device. */
int kcdc_lpt_assign(const uint64_t* lens, uint32_t nstreams, uint32_t ndev, uint32_t* dev_of);

/* ------------------------------------------- one long stream, tiled (config 3)
 * Exact intra-stream parallel CDC of a single device-resident stream: candidate
 * scan over all tiles in parallel, then chunk resolution on the device.  The
 * cut set is identical to one sequential pass (no Concatenate seams; cf.
 * snapshot/upload/upload.go:166-209, repo/object/object_manager.go:102-152).
 * `workspace` must hold kcdc_long_workspace_bytes(name, len) bytes of device
 * memory.  d_count always receives the TRUE number of chunks; entries beyond
 * `cuts_cap` are not written, so d_count > cuts_cap signals overflow (the batch
 * contract above). */
size_t kcdc_long_workspace_bytes(const char* name, uint64_t len);
int kcdc_split_long_device(const char* name, const uint8_t* d_data, uint64_t len, uint64_t* d_cuts, uint64_t cuts_cap,
                           uint64_t* d_count, void* workspace, size_t workspace_bytes, void* hip_stream);

/* ------------------------------------------- many streams of any sizes (config 5)
 * Splits n streams of arbitrary lengths (e.g. the files of one upload,
 * snapshot/upload/upload.go:769-782) with the same output contract as
 * kcdc_split_batch_device, routing each stream to the path that finishes it
 * soonest: streams that one wavefront would still be scanning after the rest
 * of the batch is done (the largest ones, >= 1 MiB) go through the long-stream
 * path, the others through one batch launch.  Boundaries are identical either
 * way.  h_dptrs (device addresses), h_lens and h_cut_base are HOST arrays;
 * d_cuts and d_counts are device memory.  Asynchronous on `hip_stream`
 * (stream-ordered allocations for scratch). */
int kcdc_split_files_device(const char* name, const uint8_t* const* h_dptrs, const uint64_t* h_lens, uint32_t n,
                            uint64_t* d_cuts, uint64_t cuts_cap, const uint64_t* h_cut_base, uint64_t* d_counts,
                            void* hip_stream);

/* ------------------------------------------------- synthetic input (bench)
 * Fill `nstreams` device streams of `stream_len` bytes each, laid out at
 * d_data + i*stride, with the counter-PRNG bytes of stream id (first_sid + i)
 * (bytes are a pure function of (seed, sid, offset); BASELINE.json configs 2-5). */
int kcdc_fill_prng(uint8_t* d_data, uint64_t stride, uint64_t stream_len, uint32_t nstreams, uint64_t seed,
                   uint64_t first_sid, void* hip_stream);

/* rand.New(rand.NewSource(seed)).Read(out[:n]) of Go math/rand: the input of
 * `kopia benchmark splitter` (cli/command_benchmark_splitters.go:66-75, one Rand
 * read block after block, so consecutive blocks are one continuous read).
 * Host-only (no GPU needed). */
int kcdc_gorand_read(int64_t seed, uint8_t* out, uint64_t n);

/* ------------------------------------------------------------- content hashes
 * The content hash Kopia computes for every chunk the splitter cuts, for many chunks of
 * device-resident bytes (repo/content/content_manager.go:812 -> repo/hashing/hashing.go:55-103).
 * Every registered name (hashing.SupportedAlgorithms(), sorted):
 *   "BLAKE2B-256", "BLAKE2B-256-128" (the default, hashing.go:51), "BLAKE2S-128", "BLAKE2S-256"
 *     keyed BLAKE2 (blake_hashes.go:8-13, truncatedKeyedHashFuncFactory);
 *   "BLAKE3-256", "BLAKE3-256-128": blake3.NewKeyed(key), key = the secret's first 32 bytes, or
 *     blake3.DeriveKey("kopia blake3 derived key v1", secret) for a shorter secret
 *     (blake3_hashes.go:10-27);
 *   "HMAC-SHA224", "HMAC-SHA256", "HMAC-SHA256-128", "HMAC-SHA3-224", "HMAC-SHA3-256":
 *     hmac.New(sha*, secret), truncated (sha_hashes.go:9-15; any key length).
 * kcdc_hash_algorithms: fills names[0..cap) and returns the count.
 * kcdc_hash_size: output bytes per chunk (16, 28 or 32), or KCDC_ENOENT.
 * kcdc_hash_chunks_device: chunk i is bytes [d_offsets[i], d_offsets[i] + d_lens[i]) of
 *   d_data (any alignment); its hash goes to d_out + i * out_stride (out_stride >= the hash
 *   size, a multiple of 4).  key: the repository's HMAC secret (<= 64 bytes for BLAKE2B,
 *   <= 32 for BLAKE2S; BLAKE2S-128 needs one, as blake2s.New128 does).  d_order: optional
 *   processing order (e.g. chunk indices by descending length: a wave runs until its
 *   longest chunk is done), NULL = as given.  Offsets, lengths and the hashes' byte counters are
 *   64 bits: neither has a limit at 2^32.  Asynchronous on hip_stream. */
int kcdc_hash_algorithms(const char** names, int cap);
int kcdc_hash_size(const char* hash_name);
int kcdc_hash_chunks_device(const char* hash_name, const uint8_t* d_data, const uint64_t* d_offsets,
                            const uint64_t* d_lens, const uint32_t* d_order, uint32_t nchunks, const uint8_t* key,
                            uint32_t key_len, uint8_t* d_out, uint32_t out_stride, void* hip_stream);

/* ------------------------------------------------------------- content encryption
 * Side channels: the AES-256-GCM kernels look up AES T-tables and GHASH tables in LDS with key- and
 * data-dependent indices (gfx950 has no AES or carry-less-multiply instructions), so they are not
 * constant-time, unlike Go's AES-NI path; use them on a single-tenant GPU.  ChaCha20-Poly1305 has no
 * table lookups.  
 * Kopia's two encryptors, AES256-GCM-HMAC-SHA256 (the default; repo/encryption/
 * aes256_gcm_hmac_sha256_encryptor.go:24-72) and CHACHA20-POLY1305-HMAC-SHA256
 * (chacha20_poly1305_hmac_sha256_encryptor.go: Encrypt/Decrypt/Overhead, 24-80; both through
 * aead_helpers.go:12-75), for many chunks per call, selected by `algorithm`:
 *   key_i  = HMAC-SHA256(secret, id_i)      id_i = the content ID the Encryptor is given; the content
 *            manager passes the last 16 bytes of the content hash (getPackedContentIV,
 *            repo/content/content_manager_lock_free.go:178-182)
 *   sealed = nonce_i(12) || AEAD(key_i, nonce_i, plaintext, aad = id_i)
 *            AEAD = AES-256-GCM (NIST SP 800-38D) or ChaCha20-Poly1305 (RFC 8439); 16-byte tag
 * secret: the repository's derived key, HKDF-SHA256(masterKey, "encryption", "", 32)
 *   (deriveKey, repo/encryption/encryption.go:80-92), 1..64 bytes.
 * kcdc_encryption_algorithms / kcdc_encryption_overhead (28): the registry (Register, encryption.go:65).
 * kcdc_crypt_workspace_size(n): bytes of device scratch a call over n chunks needs, for either
 *   algorithm (~9 KiB per chunk: its key and a table of powers of r, or of H for GCM).
 * kcdc_encrypt_chunks_device: plaintext i = [d_offsets[i], +d_lens[i]) of d_data (any
 *   alignment, < 1 GiB); d_nonces: 12 bytes per chunk (the reference draws them from
 *   crypto/rand; the caller does here); the sealed chunk (d_lens[i] + 28 bytes) is written at
 *   d_out + d_out_offsets[i] (a multiple of 4).  d_status[i]: 0, or KCDC_EFBIG (too long).
 * kcdc_decrypt_chunks_device: sealed chunk i = [d_offsets[i], +d_sealed_lens[i]) of
 *   d_sealed; its plaintext (d_sealed_lens[i] - 28 bytes) goes to d_out + d_out_offsets[i]
 *   (a multiple of 4; up to 3 zero bytes of padding after it are written too).
 *   d_status[i]: 0, KCDC_EBADMSG (authentication failed: aeadOpenPrefixedWithNonce's "unable to
 *   decrypt content"; the plaintext slot holds unauthenticated bytes), KCDC_EINVAL (shorter than
 *   28 bytes: "ciphertext too short") or KCDC_EFBIG.
 * d_ivs: iv_len (1..64) bytes per chunk at d_ivs + i * iv_stride: the content IDs (e.g. the
 * hash output of kcdc_hash_chunks_device + hash size - 16, iv_len 16).  Asynchronous on hip_stream; d_work must stay
 * allocated until the work finishes. */
int kcdc_encryption_algorithms(const char** names, int cap);
int kcdc_encryption_overhead(const char* algorithm);
uint64_t kcdc_crypt_workspace_size(uint32_t nchunks);
int kcdc_encrypt_chunks_device(const char* algorithm, const uint8_t* secret, uint32_t secret_len, const uint8_t* d_data,
                               const uint64_t* d_offsets, const uint64_t* d_lens, uint32_t nchunks,
                               const uint8_t* d_ivs, uint32_t iv_len, uint32_t iv_stride, const uint8_t* d_nonces,
                               uint8_t* d_out,
                               const uint64_t* d_out_offsets, int32_t* d_status, void* d_work, uint64_t work_bytes,
                               void* hip_stream);
int kcdc_decrypt_chunks_device(const char* algorithm, const uint8_t* secret, uint32_t secret_len,
                               const uint8_t* d_sealed, const uint64_t* d_offsets, const uint64_t* d_sealed_lens,
                               uint32_t nchunks, const uint8_t* d_ivs, uint32_t iv_len, uint32_t iv_stride,
                               uint8_t* d_out,
                               const uint64_t* d_out_offsets, int32_t* d_status, void* d_work, uint64_t work_bytes,
                               void* hip_stream);

/* ------------------------------------------------------------- content compression
 * Kopia's compressors (header IDs compression_ids.go:8-30) for many chunks per call, with the
 * content manager's keep-or-drop rule (maybeCompressAndEncryptDataForPacking,
 * repo/content/content_manager_lock_free.go:42-73):
 *   out_i = BE32(header ID) || the compressed stream of chunk i
 *   id_i  = header ID if len(out_i) < len(chunk i), else 0 (NoCompression: store chunk i as is)
 * Streams: deflate-* raw DEFLATE (RFC 1951; compressor_deflate.go:14-62), gzip* / pgzip* the same
 * stream in an RFC 1952 member with its CRC-32 and ISIZE (compressor_gzip.go:15-17,
 * compressor_pgzip.go:16-18), s2-* the S2 framing format with CRC-32C-checked chunks of Snappy
 * elements (compressor_s2.go:20-23), zstd* one RFC 8878 frame (compressor_zstd.go:15-18).  The
 * reference's readers (flate/gzip/pgzip/s2/zstd NewReader) read out_i after its 4 header bytes;
 * the bytes are this encoder's, not klauspost/compress's.
 * kcdc_compression_algorithms: the names encoded on the device; kcdc_compression_header_id: a
 *   name's header ID (or a negative error).
 * kcdc_compress_bound(len): the largest out_i for a chunk of len bytes (24 + len + 5 per 512 bytes).
 * kcdc_compress_workspace_size(total, n): device scratch for n chunks of `total` bytes in all
 *   (~1.13 bytes per input byte).
 * kcdc_compress_chunks_device: chunk i = [d_offsets[i], +d_lens[i]) of d_data (any alignment);
 *   out_i goes to d_out + d_out_offsets[i] (room for kcdc_compress_bound bytes), its length to
 *   d_out_lens[i] and id_i to d_header_ids[i].  A workspace too small for the chunks' spans
 *   leaves every d_out_lens[i] = 0.  Offsets and lengths are 64 bits with no limit at 2^32 (a
 *   gzip member's ISIZE is the length mod 2^32, RFC 1952); a call holds fewer than 2^32 spans of
 *   32 KiB.  Asynchronous on hip_stream. */
int kcdc_compression_algorithms(const char** names, int cap);
int64_t kcdc_compression_header_id(const char* algorithm);
uint64_t kcdc_compress_bound(uint64_t len);
uint64_t kcdc_compress_workspace_size(uint64_t total_bytes, uint32_t nchunks);
int kcdc_compress_chunks_device(const char* algorithm, const uint8_t* d_data, const uint64_t* d_offsets,
                                const uint64_t* d_lens, uint32_t nchunks, uint8_t* d_out,
                                const uint64_t* d_out_offsets, uint64_t* d_out_lens, uint32_t* d_header_ids,
                                void* d_work, uint64_t work_bytes, void* hip_stream);

/* ------------------------------------------------------------- content decompression
 * The read path's counterpart for many contents per call: what the committed read manager does
 * with every content whose index entry carries a compression header ID
 * (c.Decompress(output, tmp.Bytes().Reader(), true), repo/content/committed_read_manager.go:336),
 * for the s2-* compressors (s2Compressor.Decompress, compressor_s2.go:73-90: verifyCompressionHeader,
 * compressor.go:107-119, then s2.NewReader over the rest):
 *   content_i = BE32(header ID) || S2 stream      exactly what kcdc_compress_chunks_device writes
 * The stream is anything s2.NewReader accepts: the Snappy framing format (stream identifier
 * "S2sTwO" or "sNaPpY", compressed and uncompressed data chunks with the masked CRC-32C of their
 * decoded bytes, padding and skippable chunks), blocks of up to 4 MiB made of Snappy's literal,
 * copy-1, copy-2 and copy-4 elements, and S2's repeat offsets.  Every CRC is checked.
 * kcdc_decompression_algorithms: the names decoded on the device (the four s2-*).
 * kcdc_decompress_workspace_size: device scratch for nchunks contents whose output slots hold
 *   total_out_cap_bytes in all: one 32-byte block descriptor per content and one per 16 KiB of
 *   slot, plus 24 bytes per content and fixed fields.  Content i may have 1 + d_out_caps[i] / 16 KiB
 *   data chunks (writers emit blocks of 32 KiB, 64 KiB or 1 MiB), plus an equal share of whatever
 *   descriptor room a larger work_bytes gives beyond that.
 * kcdc_decompress_chunks_device: content i = [d_offsets[i], +d_comp_lens[i]) of d_comp (any
 *   alignment); its bytes go to d_out + d_out_offsets[i] (any alignment), at most d_out_caps[i] of
 *   them (the caller knows the original length from the index).  d_status[i]: 0 with
 *   d_out_lens[i] the decoded length; KCDC_EBADMSG if the first four bytes are not this name's
 *   header ID ("invalid compression header"), the framing or a block is malformed, or a CRC-32C
 *   does not match; KCDC_EOVERFLOW if the decoded length would exceed the cap; KCDC_ENOMEM if the
 *   content has more data chunks than d_work has room for.  On a failure d_out_lens[i] = 0 and
 *   the slot's contents are unspecified; no byte outside [d_out_offsets[i], +d_out_caps[i]) is
 *   written, the content's compressed bytes are read through aligned 4-byte words that hold at least
 *   one of them, and no other content of the call is affected.  d_work: 8-byte aligned.
 *   Offsets, d_comp_lens and d_out_caps are 64 bits with no limit at 2^32 (a block decodes to at
 *   most 4 MiB); a cap above 4 GiB takes the workspace kcdc_decompress_workspace_size gives for it.
 *   Returns KCDC_ENOENT for an unknown name, KCDC_EINVAL for a registered compressor with no
 *   device decoder (deflate-*, gzip*, pgzip*, zstd*).  Asynchronous on hip_stream: no host
 *   synchronisation and no copy to the host; d_work must stay allocated until the work finishes.
 *   The deflate-*, gzip* and pgzip* names are decoded by the kcdc_inflate_* family below, the
 *   zstd* names by the kcdc_zstd_decode_* family after it. */
int kcdc_decompression_algorithms(const char** names, int cap);
uint64_t kcdc_decompress_workspace_size(uint64_t total_compressed_bytes, uint64_t total_out_cap_bytes,
                                        uint32_t nchunks);
int kcdc_decompress_chunks_device(const char* algorithm, const uint8_t* d_comp, const uint64_t* d_offsets,
                                  const uint64_t* d_comp_lens, uint32_t nchunks, uint8_t* d_out,
                                  const uint64_t* d_out_offsets, const uint64_t* d_out_caps, uint64_t* d_out_lens,
                                  int32_t* d_status, void* d_work, uint64_t work_bytes, void* hip_stream);

/* ------------------------------------------------------------- inflate
 * The same step of the read path (c.Decompress, repo/content/committed_read_manager.go:336) for the
 * nine compressors whose stream is RFC 1951: deflateCompressor.Decompress
 * (compressor_deflate.go:64-78: verifyCompressionHeader, then flate.NewReader),
 * gzipCompressor.Decompress (compressor_gzip.go:68-85: gzip.NewReader) and pgzipCompressor.Decompress
 * (compressor_pgzip.go: pgzip.NewReader):
 *   content_i = BE32(header ID) || raw deflate stream                 deflate-*
 *   content_i = BE32(header ID) || RFC 1952 member(s)                  gzip*, pgzip*
 * from any writer, not only kcdc_compress_chunks_device.  A raw stream is stored, fixed and dynamic
 * blocks in any order and number, distances up to 32768 reaching back across blocks to the first
 * output byte; whatever follows its final block is ignored, as the Go reader leaves it unread.  A
 * member is 1f 8b 08, FLG with FEXTRA, FNAME, FCOMMENT and FHCRC honoured (the header CRC-16 is
 * checked), the stream, CRC-32 and ISIZE (both checked); further members may follow, as with Go's
 * multistream reader, and their output is appended; anything after a trailer that is not a whole
 * valid member is an error.  The choices made where zlib and Go's readers differ are listed in
 * kopia_amd/csrc/kcdc_inflate_format.h.
 * kcdc_inflate_algorithms: the nine names, sorted.
 * kcdc_inflate_workspace_size: device scratch for nchunks contents: a ticket and 32 bytes per
 *   content, whatever their sizes (a bit stream has no block index to make room for).
 * kcdc_inflate_chunks_device: the arguments and the contract of kcdc_decompress_chunks_device.
 *   d_status[i]: 0 with d_out_lens[i] the decoded length; KCDC_EBADMSG for a wrong header ID, a
 *   malformed stream or member, a CRC-32 or ISIZE mismatch, or truncation; KCDC_EOVERFLOW if the
 *   decoded bytes would exceed d_out_caps[i].  On a failure d_out_lens[i] = 0 and the slot's
 *   contents are unspecified; no byte outside the slot is written, compressed bytes are read through
 *   aligned 4-byte words that hold at least one byte of the content, and no other content of the
 *   call is affected.  Positions are 32 bits on the device: a content of 4 GiB or more gets
 *   KCDC_EBADMSG, and a cap above 4 GiB - 1 counts as 4 GiB - 1.  d_work: 8-byte aligned.
 *   Returns KCDC_ENOENT for an unknown name and
 *   KCDC_EINVAL for a registered name of another format (s2-*, zstd*).  nchunks == 0 launches
 *   nothing.  Asynchronous on hip_stream: no host synchronisation and no copy to the host; d_work
 *   must stay allocated until the work finishes. */
int kcdc_inflate_algorithms(const char** names, int cap);
uint64_t kcdc_inflate_workspace_size(uint32_t nchunks);
int kcdc_inflate_chunks_device(const char* algorithm, const uint8_t* d_comp, const uint64_t* d_offsets,
                               const uint64_t* d_comp_lens, uint32_t nchunks, uint8_t* d_out,
                               const uint64_t* d_out_offsets, const uint64_t* d_out_caps, uint64_t* d_out_lens,
                               int32_t* d_status, void* d_work, uint64_t work_bytes, void* hip_stream);

/* ------------------------------------------------------------- zstd decoding
 * The same step of the read path (c.Decompress, repo/content/committed_read_manager.go:336) for the
 * four zstd* compressors: zstdCompressor.Decompress (compressor_zstd.go:73-91:
 * verifyCompressionHeader, then zstd.NewReader over the rest):
 *   content_i = BE32(header ID) || RFC 8878 frames
 * from any writer, not only kcdc_compress_chunks_device, without a dictionary: any number of frames
 * with their output appended, skippable frames anywhere among them, both Single_Segment forms, every
 * Frame_Content_Size width (checked against the decoded length), Window_Descriptor from 1 KiB up,
 * a Dictionary_ID field only when it holds 0, Content_Checksum (the low 32 bits of XXH64, seed 0)
 * verified when flagged; raw, RLE and compressed blocks; Raw, RLE, Compressed and Treeless literals
 * in every size format with 1 or 4 streams; all three Number_of_Sequences encodings and the
 * Predefined, RLE, FSE_Compressed and Repeat modes of each table; repeat offsets carried across the
 * blocks of a frame.  A match offset may reach neither before its own frame's first byte nor
 * beyond Window_Size.  The choices made where libzstd and Go's reader differ are listed in
 * kopia_amd/csrc/kcdc_zstd_format.h.
 * kcdc_zstd_decode_algorithms: the four names, sorted.
 * kcdc_zstd_decode_workspace_size: device scratch for nchunks contents whose output slots hold
 *   total_out_cap_bytes in all.  Content i gets, at places fixed before any of its bytes is read:
 *   a literal room of d_out_caps[i] bytes (a content's literals cannot exceed its decoded length),
 *   a sequence room of d_out_caps[i] / 3 + 1 records of 12 bytes (every sequence yields at least 3
 *   bytes), and 4 + d_out_caps[i] / 1 KiB descriptors of 32 bytes, one per block and one per frame
 *   (1 KiB is the smallest Block_Maximum_Size), plus an equal share of whatever descriptor room a
 *   larger work_bytes gives beyond that; 36 bytes per content and fixed fields besides.
 *   Writers that fill their blocks fit; this library's own zstd-fastest frames hold a block per 512
 *   bytes and need d_out_caps[i] / 512 more descriptors for every content.
 *   total_compressed_bytes does not enter.
 * kcdc_zstd_decode_chunks_device: the arguments and the contract of kcdc_decompress_chunks_device.
 *   d_status[i]: 0 with d_out_lens[i] the decoded length; KCDC_EBADMSG for a wrong header ID, a
 *   malformed or truncated frame, a content-size or checksum mismatch; KCDC_EOVERFLOW if the decoded
 *   bytes would exceed d_out_caps[i] (a content whose headers ask for more literal or sequence room
 *   than the cap grants decodes past the cap by that fact alone); KCDC_ENOMEM if the content has
 *   more blocks and frames than its descriptors, or if work_bytes is below what
 *   kcdc_zstd_decode_workspace_size gives for the caps actually passed (then every content gets
 *   it).  On a failure d_out_lens[i] = 0 and the slot's contents are unspecified; no byte outside
 *   the slot and none outside [d_work, +work_bytes) is written, and no other content of the call is
 *   affected.  Positions are 32 bits on the device: a content of 4 GiB or more gets KCDC_EBADMSG,
 *   a cap above 4 GiB - 1 counts as 4 GiB - 1, and a content that would decode past 4 GiB - 1 gets
 *   KCDC_EOVERFLOW.  d_work: 8-byte aligned.  Returns KCDC_ENOENT for an unknown name, KCDC_EINVAL
 *   for a registered name of another format (s2-*, deflate-*, gzip*, pgzip*), a null argument, or
 *   a workspace below kcdc_zstd_decode_workspace_size(0, 0, nchunks) or misaligned, KCDC_ENODEV
 *   without a device.  nchunks == 0 launches nothing.  Asynchronous on hip_stream: no host
 *   synchronisation and no copy to the host; d_work must stay allocated until the work finishes. */
int kcdc_zstd_decode_algorithms(const char** names, int cap);
uint64_t kcdc_zstd_decode_workspace_size(uint64_t total_compressed_bytes, uint64_t total_out_cap_bytes,
                                         uint32_t nchunks);
int kcdc_zstd_decode_chunks_device(const char* algorithm, const uint8_t* d_comp, const uint64_t* d_offsets,
                                   const uint64_t* d_comp_lens, uint32_t nchunks, uint8_t* d_out,
                                   const uint64_t* d_out_offsets, const uint64_t* d_out_caps, uint64_t* d_out_lens,
                                   int32_t* d_status, void* d_work, uint64_t work_bytes, void* hip_stream);

/* ------------------------------------------------------------- error correction
 * Kopia's ECC layer for many chunks per call: repo/ecc, REED-SOLOMON-CRC32 (ecc_rs_crc.go).  A
 * repository created with an ECC overhead wraps its encryptor in encryptorWrapper
 * (repo/format/format_provider.go:115-125, encryptor_wrapper.go:13-37): every sealed chunk goes
 * through ReedSolomonCrcECC.Encrypt into a pack and through Decrypt out of it.  Stored layout
 * (ecc_rs_crc.go:157-165):
 *   ([CRC32][parity shard])+ ([CRC32][data shard])+   over   BE32(len) || chunk || zero padding
 * with IEEE CRC-32s of the zero-padded shards, big-endian, and the Reed-Solomon code of
 * klauspost/reedsolomon (go.mod:32): GF(2^8) mod 0x11d, M = V * (V[0:data])^-1, V[r][c] = r^c.
 * kcdc_ecc_algorithms / kcdc_ecc_default_algorithm: SupportedAlgorithms, ecc.go:23-35, and the one
 *   registered name (ecc_rs_crc.go:16, 414-418).
 * kcdc_ecc_params: newReedSolomonCrcECC (ecc_rs_crc.go:37-89) with computeShards
 *   (ecc_utils.go:5-20), in the reference's float32 arithmetic.  overhead_percent 1..100;
 *   max_shard_size 0 picks it by overhead (ecc_rs_crc.go:42-59), else 1..2^24.
 * kcdc_ecc_encoded_size: the exact stored size of a len-byte chunk (computeSizesFromOriginal,
 *   ecc_rs_crc.go:91-123, and Encrypt's appends); len >= 2^32 - 4 gives KCDC_EFBIG.
 * kcdc_ecc_decoded_bound: bytes of output slot a stored chunk of stored_len bytes needs
 *   (computeSizesFromStored, ecc_rs_crc.go:125-155: its data records' payload less the 4 length
 *   bytes; at least the chunk's length, at most one shard row more).
 * kcdc_ecc_matrix: the parity rows of the coding matrix, parity x data bytes, row-major
 *   (reedsolomon.New(data, parity), ecc_rs_crc.go:76-86); data + parity <= 256.
 * kcdc_ecc_workspace_size: device scratch for decoding (and repairing) nchunks stored chunks of
 *   total_stored_bytes in all: 256 bad-shard bits per block, about 5 % of the stored bytes.
 * kcdc_ecc_encode_chunks_device: Encrypt (ecc_rs_crc.go:166-250) of chunk i = [d_offsets[i],
 *   +d_lens[i]) of d_data (any alignment) to d_out + d_out_offsets[i] (any alignment, room for
 *   kcdc_ecc_encoded_size bytes).  d_status[i]: 0, or KCDC_EFBIG (nothing is written).
 *   Asynchronous on hip_stream.
 * kcdc_ecc_decode_chunks_device: Decrypt (ecc_rs_crc.go:254-350) up to ReconstructData: every
 *   stored shard's CRC is checked (the geometry comes from d_stored_lens[i] alone; bytes past the
 *   stored end read as zeros and data shards that start there are not checked, :297-303), the data
 *   shards' payload goes to d_out + d_out_offsets[i] (room for kcdc_ecc_decoded_bound bytes; bytes
 *   past d_out_lens[i] hold padding) and the failed shards of every block are recorded in d_work.
 *   d_status[i]: 0 with d_out_lens[i] the in-band length; KCDC_ECC_DAMAGED if a checked shard
 *   failed (d_out_lens[i] = 0, the slot holds unverified bytes: call the repair);
 *   KCDC_EBADMSG if the in-band length exceeds what the stored bytes hold (slot zeroed);
 *   KCDC_EINVAL if stored_len < 40, the smallest stored size; KCDC_ENOMEM if d_work is too
 *   small for the chunk's blocks.  Offsets and stored lengths are 64 bits with no limit at 2^32
 *   (the in-band length is below it by construction); the host's kcdc_ecc_decoded_bound refuses a
 *   stored_len above 2^40 with KCDC_EFBIG, the device call has no check of its own there.
 *   Asynchronous on hip_stream.
 * kcdc_ecc_repair_chunks_device: ReconstructData (ecc_rs_crc.go:325) for the chunks a decode call
 *   with the same arguments left KCDC_ECC_DAMAGED.  Waits for hip_stream, reads back the statuses
 *   and the bad-shard masks, inverts one matrix per erasure pattern on the host, rebuilds the
 *   missing data shards in the output slots on the device and sets status 0 and d_out_lens[i]; a
 *   chunk with a block that lost more than its parity shards gets KCDC_EBADMSG and a zeroed slot
 *   ("Error computing ECC", :326-328).  No-op when no chunk is damaged.  Synchronises hip_stream. */
#define KCDC_ECC_DAMAGED 1 /* d_status of a decoded chunk with failed shards, before the repair */
typedef struct kcdc_ecc_info {
    int32_t data_shards, parity_shards, max_shard_size;
    int32_t threshold_parity_input, threshold_parity_output, threshold_blocks_input, threshold_blocks_output;
} kcdc_ecc_info;
int kcdc_ecc_algorithms(const char** names, int cap);
const char* kcdc_ecc_default_algorithm(void);
int kcdc_ecc_params(const char* algorithm, int32_t overhead_percent, int32_t max_shard_size, kcdc_ecc_info* out);
int64_t kcdc_ecc_encoded_size(const char* algorithm, int32_t overhead_percent, int32_t max_shard_size, uint64_t len);
int64_t kcdc_ecc_decoded_bound(const char* algorithm, int32_t overhead_percent, int32_t max_shard_size,
                               uint64_t stored_len);
int kcdc_ecc_matrix(int32_t data_shards, int32_t parity_shards, uint8_t* out);
uint64_t kcdc_ecc_workspace_size(uint64_t total_stored_bytes, uint32_t nchunks);
int kcdc_ecc_encode_chunks_device(const char* algorithm, int32_t overhead_percent, int32_t max_shard_size,
                                  const uint8_t* d_data, const uint64_t* d_offsets, const uint64_t* d_lens,
                                  uint32_t nchunks, uint8_t* d_out, const uint64_t* d_out_offsets, int32_t* d_status,
                                  void* hip_stream);
int kcdc_ecc_decode_chunks_device(const char* algorithm, int32_t overhead_percent, int32_t max_shard_size,
                                  const uint8_t* d_stored, const uint64_t* d_offsets, const uint64_t* d_stored_lens,
                                  uint32_t nchunks, uint8_t* d_out, const uint64_t* d_out_offsets,
                                  uint64_t* d_out_lens, int32_t* d_status, void* d_work, uint64_t work_bytes,
                                  void* hip_stream);
int kcdc_ecc_repair_chunks_device(const char* algorithm, int32_t overhead_percent, int32_t max_shard_size,
                                  const uint8_t* d_stored, const uint64_t* d_offsets, const uint64_t* d_stored_lens,
                                  uint32_t nchunks, uint8_t* d_out, const uint64_t* d_out_offsets,
                                  uint64_t* d_out_lens, int32_t* d_status, void* d_work, uint64_t work_bytes,
                                  void* hip_stream);

/* ------------------------------------------------------------- packing
 * What the content manager does with a new content between the cut and the pack blob
 * (maybeCompressAndEncryptDataForPacking, repo/content/content_manager_lock_free.go:30-89, and the
 * append of addToPackUnlocked, content_manager.go:257-353), for many chunks per call with no host
 * round trip between the stages.  Per content, in order:
 *   1. compress (if `compression` is set): out = BE32(header ID) || stream, kept iff
 *      len(out) < len(chunk); otherwise the header ID is 0 and the original is used
 *      (kcdc_compress_chunks_device);
 *   2. seal with `encryption`, IV = the content ID, nonce from the caller
 *      (kcdc_encrypt_chunks_device);
 *   3. wrap with `ecc` if set (kcdc_ecc_encode_chunks_device);
 *   4. append to the pack: PackOffset = the pack's length, PackedLength = the stored length; a pack
 *      whose length is >= max_pack_size after the append is closed and the next content opens a new
 *      one, whose length starts at pack_lead (content_manager.go:314-334).
 * The dedup decision is d_keep, the host's or kcdc_dedup_claim_device's (below).  The host keeps
 * blob IDs, the preamble's bytes, the postamble, the index and the split by pack prefix: one call
 * packs the contents of one prefix.
 * kcdc_pack_params: max_pack_size 1..2^30; pack_lead: bytes left free at the head of every new pack
 *   (the host fills them); open_fill: 0, or the length (< max_pack_size) of an open pack that pack 0
 *   of this call continues; max_total_bytes (<= 2^40): the caller's bound on the sum of the packed
 *   chunks' lengths, which sizes the workspace.
 * kcdc_pack_bounds: for nchunks chunks under these parameters, the bytes of d_pack, the rows of
 *   d_packs and the bytes of d_work that no call can exceed.
 * kcdc_pack_chunks_device: chunk i = [d_offsets[i], +d_lens[i]) of d_data (any alignment);
 *   d_keep[i] == 0 leaves chunk i out (NULL: all are packed); d_ids / d_nonces as
 *   kcdc_encrypt_chunks_device's d_ivs / d_nonces.
 *   Layout of d_pack: pack 0 starts at 0 and pack k+1 at pack k's end rounded up to 256; the bytes of
 *   pack k from pack offset x on are at d_packs[k].start + x, x >= pack_lead (open_fill for pack 0
 *   when it is non-zero).  The lead bytes and the gaps are never written.  A pack exists only if a
 *   content went into it; only the last may be open (length < max_pack_size).
 *   d_entries[i].status: 0 packed; KCDC_PACK_SKIPPED (d_keep[i] == 0) and KCDC_EFBIG (longer than
 *   the seal's limit, 2^30 - 64) take no room.  Decided on the device for the whole call, with
 *   d_totals = {0, 0} and no byte of d_pack written: KCDC_ENOMEM in every entry if the packed
 *   lengths sum to more than max_total_bytes, KCDC_EOVERFLOW if the packs do not fit pack_cap or
 *   packs_cap (neither arises with buffers sized by kcdc_pack_bounds from a true max_total_bytes).
 *   d_totals[0]: packs; d_totals[1]: bytes of d_pack used (the last pack's end).  Rows of d_packs
 *   from d_totals[0] on are not written, except that a KCDC_EOVERFLOW call may leave the rows it
 *   placed before it refused (never more than packs_cap).
 *   d_work: 256-byte aligned, work_bytes >= kcdc_pack_bounds'.  Asynchronous on hip_stream: no host
 *   synchronisation, allocation or copy; every array is device memory and must stay allocated until
 *   the work finishes.  nchunks == 0 only zeroes d_totals.
 *   Returns KCDC_ENOENT (unknown name), KCDC_EINVAL (bad parameter, null argument, misaligned or
 *   short workspace) or KCDC_ENODEV before anything is launched. */
#define KCDC_PACK_SKIPPED 1
typedef struct kcdc_pack_params {
    const char* compression;      /* a kcdc_compression_algorithms name, or NULL: NoCompression */
    const char* encryption;       /* a kcdc_encryption_algorithms name */
    const uint8_t* secret;
    uint32_t secret_len;
    const char* ecc;              /* NULL: none, else a kcdc_ecc_algorithms name */
    int32_t ecc_overhead_percent, ecc_max_shard_size;
    uint64_t max_pack_size;
    uint32_t pack_lead;
    uint32_t open_fill;
    uint64_t max_total_bytes;
} kcdc_pack_params;
typedef struct kcdc_pack_entry { /* 24 bytes, one per chunk: the Info fields the device decides */
    uint32_t pack, pack_offset, packed_length, original_length, header_id;
    int32_t status;
} kcdc_pack_entry;
typedef struct kcdc_pack_info { /* 24 bytes, one per pack */
    uint64_t start, length;     /* place in d_pack; the pack's length, lead / open_fill included */
    uint32_t first, count;      /* its contents are the count packed chunks from chunk index first on */
} kcdc_pack_info;
int kcdc_pack_bounds(const kcdc_pack_params* params, uint32_t nchunks, uint64_t* pack_bytes, uint32_t* max_packs,
                     uint64_t* work_bytes);
int kcdc_pack_chunks_device(const kcdc_pack_params* params, const uint8_t* d_data, const uint64_t* d_offsets,
                            const uint64_t* d_lens, const uint8_t* d_keep, uint32_t nchunks, const uint8_t* d_ids,
                            uint32_t id_len, uint32_t id_stride, const uint8_t* d_nonces, uint8_t* d_pack,
                            uint64_t pack_cap, kcdc_pack_entry* d_entries, kcdc_pack_info* d_packs,
                            uint32_t packs_cap, uint64_t* d_totals, void* d_work, uint64_t work_bytes,
                            void* hip_stream);

/* ------------------------------------------------------------- content dedup
 * WriteContent's lookup between hashData and addToPackUnlocked (repo/content/content_manager.go:
 * 812-842) on the device: a set of content IDs in device memory, and a claim call that turns a batch
 * of digests into the d_keep mask kcdc_pack_chunks_device takes, with no host round trip.
 * A key is `prefix` (the content ID's one-letter prefix, index.IDPrefix; 0 for none) and id_len hash
 * bytes at d_ids + i * id_stride (any alignment, id_stride >= id_len).  id_len is fixed per set,
 * 16..32 (every kcdc_hash_size).  Two keys are equal iff the prefix and all id_len bytes are equal.
 * kcdc_dedup_new: a set for up to max_keys (1..2^31) keys on `device`; all device memory the set
 *   ever uses, kcdc_dedup_bytes(id_len, max_keys), is allocated here.  NULL + kcdc_last_error.
 * kcdc_dedup_claim_device: the WriteContent decision, as if the n IDs were presented one after
 *   another in index order.  d_keep[i] = 1 iff the key was not in the set before the call and no
 *   j < i of the call has an equal key, else 0.  d_first[i] (may be NULL): the lowest index of the
 *   call with an equal key (i itself exactly when d_keep[i] == 1), or KCDC_DEDUP_KNOWN if the key
 *   was in the set before the call.  After the call every distinct key of the call is in the set.
 *   d_totals[0]: the call's status (0, or KCDC_ENOSPC as a 64-bit two's complement value);
 *   d_totals[1]: keys newly stored; d_totals[2]: keys stored in all.  The results are a function of
 *   the set's contents and the ID array alone, whatever the grid and the scheduling.
 * kcdc_dedup_insert_device: claim without the per-ID outputs, for loading the committed index.  The
 *   host leaves deleted entries out, so a deleted content is written again
 *   (content_manager.go:825-840).
 * kcdc_dedup_lookup_device: d_known[i] = 1 iff the key is in the set, else 0; the set is unchanged.
 * kcdc_dedup_grow_device: inserts every key of `from` into `to` (same id_len, same device): the
 *   way to enlarge a full set.  `from` is unchanged.
 * kcdc_dedup_clear_device: empties the set.
 * kcdc_dedup_count: keys stored, after waiting for hip_stream; or a negative KCDC_E* code.
 * Refusal, decided on the device for the whole call: claim, insert and grow are refused if the keys
 *   stored plus n (grow: plus the keys of `from`) exceed max_keys, whether or not some of the IDs
 *   are duplicates, so the host can predict it.  A refused call changes nothing in the set and
 *   gives d_totals = {KCDC_ENOSPC, 0, keys stored}, every d_keep[i] = 0 and every d_first[i] =
 *   KCDC_DEDUP_KNOWN.  No partial insert is ever visible.
 * Every *_device call is asynchronous on hip_stream: no host synchronisation, allocation or copy;
 *   every array is device memory and must stay allocated until the work finishes.  n == 0 launches
 *   nothing but writes d_totals.  Calls on one set (for grow: on either set) must be ordered by the
 *   caller, on one stream or by events: the set does no locking, and two calls in flight on one set
 *   corrupt it.  Different sets are independent.
 *   Returns KCDC_EINVAL (null argument, id_len outside 16..32, id_stride < id_len, max_keys 0 or
 *   above 2^31, mismatched sets), KCDC_ENOMEM or KCDC_ENODEV before anything is launched.
 * kcdc_test_dedup_home (test hook, host arithmetic): the first slot probed for a key in a set of
 *   this shape; UINT64_MAX for a bad shape. */
typedef struct kcdc_dedup kcdc_dedup;
#define KCDC_DEDUP_KNOWN UINT32_MAX /* d_first[i]: the ID was in the set before this call */
kcdc_dedup* kcdc_dedup_new(int device, uint32_t id_len, uint64_t max_keys);
void kcdc_dedup_free(kcdc_dedup* t);
uint64_t kcdc_dedup_bytes(uint32_t id_len, uint64_t max_keys); /* device memory a set takes (0: bad shape); host only */
int64_t kcdc_dedup_count(kcdc_dedup* t, void* hip_stream);
int kcdc_dedup_clear_device(kcdc_dedup* t, void* hip_stream);
int kcdc_dedup_claim_device(kcdc_dedup* t, uint8_t prefix, const uint8_t* d_ids, uint32_t id_stride, uint32_t n,
                            uint8_t* d_keep, uint32_t* d_first, uint64_t* d_totals, void* hip_stream);
int kcdc_dedup_insert_device(kcdc_dedup* t, uint8_t prefix, const uint8_t* d_ids, uint32_t id_stride, uint32_t n,
                             uint64_t* d_totals, void* hip_stream);
int kcdc_dedup_lookup_device(kcdc_dedup* t, uint8_t prefix, const uint8_t* d_ids, uint32_t id_stride, uint32_t n,
                             uint8_t* d_known, void* hip_stream);
int kcdc_dedup_grow_device(kcdc_dedup* from, kcdc_dedup* to, uint64_t* d_totals, void* hip_stream);
uint64_t kcdc_test_dedup_home(uint32_t id_len, uint64_t max_keys, uint8_t prefix, const uint8_t* id);

/* ------------------------------------------------------------- testing
 * Hooks for the library's own tests (not part of the splitter surface).
 * kcdc_test_set: process-wide knobs read by every later batch launch.
 *   KCDC_TEST_SPIN_CAP    polls with no stream finishing before a waiting wave gives up, the
 *                         current poll included (0: default, ~seconds; 1: at the first
 *                         unready poll)
 *   KCDC_TEST_NO_STEAL    1: waves never requeue the streams of workgroups that have not started
 *   KCDC_TEST_FORCE_ERROR 1: every batch launch reports failure (KCDC_COUNT_FAILED)
 *   KCDC_TEST_HASH_LANES  lanes per chunk of kcdc_hash_chunks_device: 0 auto (4 up to 2^20
 *                         chunks, else 1), 1 or 4
 *   KCDC_TEST_NO_SERVER   1: private streaming handles launch one scan per call instead of using
 *                         the device's resident scan server
 *   KCDC_TEST_NO_HELP     1: batch launches without intra-region help (each region is scanned by
 *                         the wave that owns its stream only); 2: help on whatever the average
 *                         (0, the default: help for averages of 1 MiB and up, and for Rabin-Karp
 *                         launches with fewer streams than waves)
 *   KCDC_TEST_ID_RING     bytes of the writers' content-ID ring for batchers created from now on
 *                         (0: the default; small values exercise wrap-around and backpressure)
 *   KCDC_TEST_LANE_CAP    buzhash batch launches: bytes per lane segment (a tile is 64 of them),
 *                         a power of two in [256, 4096]; 0: the default (avg / 256 within
 *                         [256, 2048]).  Other tile geometries for the same cuts.
 *   KCDC_TEST_HELP_WINDOW both batch kernels: tiles of a region published to helpers at a time,
 *                         in [3, 254]; 255: whole regions; 0: the default (the launch's rule)
 *   KCDC_TEST_PAR_NODE_CAP long-stream launches (and their workspace sizes): nodes of the parallel
 *                         resolver's tables per launch, in [1, 2^20]; 0: the default (2^20).  A
 *                         stream whose nodes do not fit resolves serially, with the same cuts.
 *   KCDC_TEST_LONG_STAT   1: every long-stream launch records which resolver took each of its
 *                         streams, for kcdc_test_long_stat
 *   KCDC_TEST_DEFLATE_MAXB the deflate family's launches: the longest literal/length and distance
 *                         code of a dynamic block, in [9, 15]; 0: the default (15, RFC 1951's limit).
 *                         A lower limit gives a valid stream and makes the length limiter run on
 *                         ordinary skewed data.
 *   KCDC_TEST_DEFLATE_CL_MAXB the same for the dynamic header's code-length code, in [5, 7]; 0: the
 *                         default (7)
 *   KCDC_TEST_CHUNK_GRID  the most workgroups the persistent per-chunk kernels are launched with:
 *                         the unit passes of kcdc_encrypt / kcdc_decrypt_chunks_device, the block
 *                         decode of kcdc_decompress_chunks_device and the content decode of
 *                         kcdc_inflate_chunks_device (their CRC passes follow), and the entropy and
 *                         execute passes of kcdc_zstd_decode_chunks_device (zstd_entropy_kernel,
 *                         zstd_execute_kernel; its checksum pass follows), and the probe, outcome,
                         commit and lookup kernels of kcdc_dedup_*; 0: the default (no
 *                         cap); negative: KCDC_EINVAL.  Same results from any grid: with one
 *                         workgroup a few hundred tiny chunks make every wave walk many chunks and
 *                         take many tickets, which otherwise needs tens of thousands.
 * kcdc_test_long_stat: after the last long-stream launch made with KCDC_TEST_LONG_STAT on has
 * finished (synchronise first): KCDC_TEST_LONG_STREAMS, the streams of that launch, or
 * KCDC_TEST_LONG_SERIAL, how many of them the serial resolver took (truncated segments, or no
 * room in the node tables); the parallel resolver took the others.  Negative KCDC_E* code if no
 * launch was recorded.
 * kcdc_test_occupy: occupy `nwg` CUs (one workgroup with all of the CU's LDS each) for
 * `usec` microseconds on `hip_stream`, e.g. to run a batch beside a kernel that holds CUs.
 * kcdc_test_queue_stat: after the last pipelined batch launch has finished (synchronise
 * first), read one word of its queue header: KCDC_TEST_STAT_GIVEUPS (waves that gave up
 * waiting), KCDC_TEST_STAT_DONE (streams finished), KCDC_TEST_STAT_STEALS (requeued
 * workgroups), KCDC_TEST_STAT_HELPS (tiles scanned by waves that helped another wave's region),
 * KCDC_TEST_STAT_TICKETS / KCDC_TEST_STAT_ENTRIES (the ring's ticket and entry counters) and
 * KCDC_TEST_STAT_WAVES (the launch's waves).  Every wave exits holding one ticket and every
 * reserved entry is written, so TICKETS - ENTRIES is WAVES (WAVES - 1 when the last stream's
 * final entry is a tombstone nobody waited for).  Synchronous copy; returns the word, or a
 * negative KCDC_E* code.
 * kcdc_test_batch_plan: what a batch launch of `nstreams` streams of splitter `algorithm` on
 * device 0 would run with, the knobs above as they stand: out[0] the bytes per lane segment (the
 * buzhash kernel's; a Rabin-Karp lane is twice that), out[1] whether waiting waves help (0/1),
 * out[2] the help window in tiles (0: whole regions), out[3] the launch's waves.  Host code only,
 * nothing is launched; the tests' tile model checks itself against it.  0, or a negative KCDC_E*
 * code (unknown or fixed-size splitter, no streams, no device). */
#define KCDC_TEST_SPIN_CAP 1
#define KCDC_TEST_NO_STEAL 2
#define KCDC_TEST_FORCE_ERROR 3
#define KCDC_TEST_HASH_LANES 4
#define KCDC_TEST_NO_SERVER 5
#define KCDC_TEST_NO_HELP 6
#define KCDC_TEST_ID_RING 7
#define KCDC_TEST_LANE_CAP 8
#define KCDC_TEST_HELP_WINDOW 9
#define KCDC_TEST_PAR_NODE_CAP 10
#define KCDC_TEST_LONG_STAT 11
#define KCDC_TEST_DEFLATE_MAXB 12
#define KCDC_TEST_DEFLATE_CL_MAXB 13
#define KCDC_TEST_CHUNK_GRID 14
int kcdc_test_set(int32_t key, int64_t value);
#define KCDC_TEST_LONG_STREAMS 1
#define KCDC_TEST_LONG_SERIAL 2
int64_t kcdc_test_long_stat(int32_t key);
int kcdc_test_occupy(uint32_t nwg, uint32_t usec, void* hip_stream);
#define KCDC_TEST_STAT_GIVEUPS 1
#define KCDC_TEST_STAT_DONE 2
#define KCDC_TEST_STAT_STEALS 3
#define KCDC_TEST_STAT_HELPS 4
#define KCDC_TEST_STAT_TICKETS 10
#define KCDC_TEST_STAT_ENTRIES 11
#define KCDC_TEST_STAT_WAVES 12
int64_t kcdc_test_queue_stat(int32_t key);
int kcdc_test_batch_plan(const char* algorithm, uint32_t nstreams, uint32_t out[4]);
/* Test hook: copy bytes [off, off + n) of the last pipelined launch's queue workspace (queue
 * header, stream ring, help slots) to host memory at dst; 0 or a negative error. */
int kcdc_test_ws_copy(void* dst, uint64_t off, uint64_t n);
/* Requests the resident scan server has answered in this process (private streaming handles use
 * it while exactly one private handle is open). */
int64_t kcdc_test_server_requests(void);

#ifdef __cplusplus
}
#endif
#endif /* KCDC_H */
